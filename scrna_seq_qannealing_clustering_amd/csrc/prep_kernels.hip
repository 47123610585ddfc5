// prep_kernels.hip -- counts -> log-normalised matrix -> gene statistics -> scaled matrix -> Gram matrix / projection (gfx950).
// C ABI, layouts and LDS plans: include/mi_prep.h; the loess curve and the eigen-solve are host fp64 in preprocess.py.
//
//   k_prep_normalize     one wavefront per cell: fp64 total, then y = (float) log1p((double) x * scale / total).
//   k_prep_col_partial<Mode>  per-column reductions over a slice of kRowSlice rows, 64 columns x 4 row lanes per workgroup.  The
//                        mode is the term: ColSum (sum and non-zero count), ColLog1p, ColCentred (squares about a given
//                        mean), ColClipped (vst's clipped standardised squares), RegressMoment and SctMoment (a residual, or
//                        its square about a mean); k_prep_col_finish adds the slices in ascending order and divides.
//   k_prep_select        z = fminf((y - mu) * inv, clip) for the chosen columns, into Z (n x ldz, zero padded columns);
//                        k_sct_select: the clipped Pearson residual instead.
//   k_prep_gram          one (upper-triangle 128 x 128 tile, chunk of kChunk cells) per workgroup on the f32-input MFMA,
//                        f32 tile out; k_prep_gram_reduce adds the chunks in fp64 in chunk order and mirrors.
//   k_prep_project       out = Z V, 64 cells x 128 columns per workgroup on the same MFMA.
//   k_prep_cell_qc       per cell: the normaliser's fp64 total, the total of a gene subset, the count of x != 0.
//   k_prep_regress_*     mi_prep_select_regressed on the gathered Z: c = Q^T y and sum y^2 (coef) and the in-place scaling
//                        (scale), on the slices, lanes and LDS join of k_prep_col_partial, fp64, no contraction.
//   k_sct_*              SCTransform: the gather of the fit block, dense and sparse, and the per-gene negative-binomial fit
//                        (one workgroup per gene, its counts in LDS); the corrected counts and the data slot as a second
//                        handle (k_sct_correct, k_sct_csr_rows), whose sparse structure is built on the device.
// A sparse handle (mi_prep_create_csr_f32) keeps the counts as CSR and is served by k_prep_csr_normalize,
// k_prep_csc_col_partial<Term> (k_prep_csc_row_partial<Mode> for the SCT residuals), k_prep_csr_select<Cols> and
// k_prep_csr_cell_qc, which add in the order of their dense kernels and call the same term functions, on 0.0f for a zero:
// the same bits come out.
// Operand maps of v_mfma_f32_32x32x2_f32 as in energy_kernels.hip: A: lane l holds A[i = l & 31][k = l >> 5]; B: lane l
// holds B[k = l >> 5][j = l & 31]; C/D: register q of lane l is C[row = (q & 3) + 8 (q >> 2) + 4 (l >> 5)][col = l & 31].
// No floating-point atomics; stores are ordinary vector stores.
#include <algorithm>
#include <memory>
#include <vector>

#include "../../include/mi_prep.h"
#include "mi_prep_csr.h"
#include "mi_prep_handle.h"
#include "mi_sa_device.h"
#include "mi_sct_math.h"

namespace mi_sa_impl {
namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kRowSlice = MI_PREP_ROW_SLICE;
constexpr int kChunk = MI_PREP_GRAM_CHUNK;
constexpr int kTile = 128, kKC = 32;
constexpr int kProjCells = 64, kProjCols = MI_PREP_MAX_PCS;
constexpr size_t kGramWorkspace = (size_t)MI_PREP_GRAM_WORKSPACE;                // bytes of f32 tiles in flight between the two Gram kernels
constexpr int kMaxQ = MI_PREP_MAX_DESIGN_COLS;

__global__ void __launch_bounds__(256) k_prep_normalize(const float *__restrict__ X, float *__restrict__ Y, int n, int g,
                                                        double scale)
{
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (size_t)n) return;
    const float *x = X + row * g;
    float *y = Y + row * g;
    double t = 0.0;
    for (int j = lane; j < g; j += 64) t += (double)x[j];
    t = wave_sum_f64(t);
    for (int j = lane; j < g; j += 64) y[j] = t > 0.0 ? (float)log1p((double)x[j] * scale / t) : 0.0f;
}

// ---- the column reductions: every term is written once, and so is the skeleton of each source form -------------------------
// A workgroup is 64 columns x 4 row lanes over a slice of kRowSlice rows: lane ty adds the rows r0 + ty, r0 + ty + 4, ...
// ascending, the four lanes meet in LDS as ((s0 + s1) + s2) + s3, and k_prep_col_finish adds the slices in ascending order
// and divides once.  All of it is fp64 without contraction: every product is a multiply, then an add.
//
// A mode is the kernel argument that says what is added: `count` columns are reduced, bind(j) loads what column j needs and
// returns its column in the source, and mode(v, r) is the term of value v in row r.  The dense kernel applies it to every
// element; the transposed kernels apply the same term to the stored values and to 0.0f for a zero, at that row's place
// in the order, so a sparse handle gives the bits of a dense one.  kWalk says which zeros a transposed kernel may skip.
enum { kWalkStored,        // a zero's term is +0.0 (and the sum is never negative): the stored entries alone
       kWalkZeroConstant,  // a zero's term is one constant per gene, hoisted and added for each run of zeros
       kWalkEveryRow };    // a zero's term depends on the row: every row is computed

// the tail of the moment modes: the value itself (MODE 0) or its square about a mean (MODE 1)
template <int MODE>
__device__ __forceinline__ double moment_tail(double x, double mean)
{
    if (!MODE) return x;
    const double d = x - mean;
    return d * d;
}

// The four terms over the counts and the normalised values.  term(v, mj, sj, clip) is the arithmetic, written here alone.
struct SumTerm {                                                  // the sum, and the count of v != 0
    static constexpr int kWalk = kWalkStored;
    static constexpr bool kCounts = true, kUsesMean = false, kUsesSd = false;
    static __device__ __forceinline__ double term(float v, double, double, double) { return (double)v; }
};

struct Log1pTerm {                                                // (log1p(0) is +0.0, like the 0 of a sum)
    static constexpr int kWalk = kWalkStored;
    static constexpr bool kCounts = false, kUsesMean = false, kUsesSd = false;
    static __device__ __forceinline__ double term(float v, double, double, double) { return log1p((double)v); }
};

struct CentredTerm {                                              // squares about a given mean
    static constexpr int kWalk = kWalkZeroConstant;
    static constexpr bool kCounts = false, kUsesMean = true, kUsesSd = false;
    static __device__ __forceinline__ double term(float v, double mj, double, double) { return moment_tail<1>((double)v, mj); }
};

struct ClippedTerm {                                              // vst's clipped standardised squares (sj != 0)
    static constexpr int kWalk = kWalkZeroConstant;
    static constexpr bool kCounts = false, kUsesMean = true, kUsesSd = true;
    static __device__ __forceinline__ double term(float v, double mj, double sj, double clip)
    {
        double d = ((double)v - mj) / sj;
        d = d < clip ? d : clip;
        return d * d;
    }
};

// the mode of one of these terms: mean, sd and clip as far as the term uses them
template <typename T>
struct ColMode {
    typedef T Term;
    static constexpr int kWalk = T::kWalk;
    static constexpr bool kCounts = T::kCounts;
    int count;
    const double *mean, *sd;
    double clip, mj, sj;
    __device__ int bind(int j)
    {
        if (T::kUsesMean) mj = mean[j];
        if (T::kUsesSd) sj = sd[j];
        return j;
    }
    // (a gene without spread adds +0.0 to a sum of squares)
    __device__ double operator()(float v, int) const { return !T::kUsesSd || sj != 0.0 ? T::term(v, mj, sj, clip) : 0.0; }
};
typedef ColMode<SumTerm> ColSum;
typedef ColMode<Log1pTerm> ColLog1p;
typedef ColMode<CentredTerm> ColCentred;
typedef ColMode<ClippedTerm> ColClipped;

// One gathered column of mi_prep_select_regressed: r = y - sum_k Q_ik c_k, as acc = Q_i0 c_0, then acc = acc + Q_ik c_k for
// k ascending.  Q: n x q row-major fp64 (q <= kMaxQ); the row lane is one wavefront, so its row of Q comes by scalar loads.
struct RegressColumn {
    const double *Q;
    int q;
    const double *coef;                                           // q x h
    double c[kMaxQ];
    __device__ void bind(int j, int h)
    {
#pragma unroll
        for (int k = 0; k < kMaxQ; ++k) c[k] = k < q ? coef[(size_t)k * h + j] : 0.0;
    }
    __device__ double residual(float y, int r) const
    {
        const double *qr = Q + (size_t)r * q;
        double acc = qr[0] * c[0];
#pragma unroll
        for (int k = 1; k < kMaxQ; ++k)
            if (k < q) acc = acc + qr[k] * c[k];
        return (double)y - acc;
    }
};

template <int MODE>
struct RegressMoment {                                            // the regression residuals' sum, or squares about their mean
    static constexpr bool kCounts = false;
    int count;
    RegressColumn col;
    const double *mean;
    double mj;
    __device__ int bind(int j)
    {
        col.bind(j, count);
        mj = MODE ? mean[j] : 0.0;
        return j;
    }
    __device__ double operator()(float v, int r) const { return moment_tail<MODE>(col.residual(v, r), mj); }
};

// the Pearson residual of count x under mu = exp(b0 + b1 log_umi), variance mu + alpha mu^2, clipped to +- clip
__device__ __forceinline__ double sct_residual(float x, double b0, double b1, double alpha, double lu, double clip)
{
    const double mu = exp(b0 + b1 * lu);
    const double r = ((double)x - mu) / sqrt(mu + alpha * (mu * mu));
    return fmin(fmax(r, -clip), clip);
}

template <int MODE>
struct SctMoment {                                                // the Pearson residuals' sum, or squares about their mean
    static constexpr int kWalk = kWalkEveryRow;
    static constexpr bool kCounts = false;
    int count;
    const int32_t *genes;
    const double *par, *lu;                                       // par: b0, b1, alpha, `count` entries each; lu: per cell
    double clip;
    const double *mean;
    double b0, b1, al, mj;
    __device__ int bind(int jj)
    {
        b0 = par[jj];
        b1 = par[count + jj];
        al = par[2 * (size_t)count + jj];
        mj = MODE ? mean[jj] : 0.0;
        return genes[jj];
    }
    __device__ double operator()(float v, int r) const { return moment_tail<MODE>(sct_residual(v, b0, b1, al, lu[r], clip), mj); }
};

// this thread's place in the skeleton: column j (tx) of the reduction, row lane ty, the slice's rows [r0, r1)
struct ColSlice {
    const int tx = threadIdx.x & 63, ty = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int j = blockIdx.x * 64 + tx;
    const int r0 = blockIdx.y * kRowSlice, r1;
    __device__ explicit ColSlice(int n) : r1(r0 + kRowSlice < n ? r0 + kRowSlice : n) {}
    // the four lanes' values of a column meet in LDS, joined left to right; lane 0 stores for the columns that exist
    template <typename T>
    __device__ void join(T v, bool live, T *out) const
    {
        __shared__ T s[4][64];
        s[ty][tx] = v;
        __syncthreads();
        if (ty == 0 && live) *out = ((s[0][tx] + s[1][tx]) + s[2][tx]) + s[3][tx];
    }
    // the end of a reduction over `count` columns: the partial of (slice, column) at slice * count + j
    template <typename Mode>
    __device__ void store(const Mode &mode, double acc, int32_t cnt, double *psum, int32_t *pnnz) const
    {
        const size_t o = (size_t)blockIdx.y * mode.count + j;
        join(acc, j < mode.count, psum + o);
        if (Mode::kCounts) join(cnt, j < mode.count, pnnz + o);
    }
};

// the dense source: M is n x ld row-major
template <typename Mode>
__global__ void __launch_bounds__(256) k_prep_col_partial(const float *__restrict__ M, int ld, int n, Mode mode,
                                                          double *__restrict__ psum, int32_t *__restrict__ pnnz)
{
    const ColSlice s(n);
    double acc = 0.0;
    int32_t cnt = 0;
    if (s.j < mode.count) {
        const float *col = M + mode.bind(s.j);
        for (int r = s.r0 + s.ty; r < s.r1; r += 4) {
            const float v = col[(size_t)r * ld];
            acc += mode(v, r);
            if (Mode::kCounts) cnt += v != 0.0f;
        }
    }
    s.store(mode, acc, cnt, psum, pnnz);
}

__global__ void __launch_bounds__(256) k_prep_col_finish(const double *__restrict__ psum, const int32_t *__restrict__ pnnz,
                                                         int slices, int g, double denom, double *__restrict__ out,
                                                         int32_t *__restrict__ out_nnz)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= g) return;
    double t = 0.0;
    int32_t c = 0;
    for (int s = 0; s < slices; ++s) {
        t += psum[(size_t)s * g + j];
        if (pnnz) c += pnnz[(size_t)s * g + j];
    }
    out[j] = t / denom;
    if (pnnz) out_nnz[j] = c;
}

// ---- the selections into Z (n x ldz, h chosen columns, zero padding) --------------------------------------------------------
// `cols` says what column c of Z holds for input x; bind_row(row) loads what a cell needs: the argument of the CSR kernel
// below, which applies it to 0.0f for what a cell does not store.  The two dense kernels take the same fields one by one
// and call the same scaled_value / sct_residual.
// mi_prep_select's scaling, as separate f32 operations
__device__ __forceinline__ float scaled_value(float y, float mu, float inv, float clip)
{
    const float d = y - mu;
    return fminf(d * inv, clip);
}

struct ScaledCols {                                               // mi_prep_select: z = fminf((y - mu) * inv, clip), 0 where flat
    int h;
    const float *mu, *inv;
    const uint8_t *flat;
    float clip;
    __device__ void bind_row(size_t) {}
    __device__ float operator()(int c, float y) const
    {
        return c < h && !flat[c] ? scaled_value(y, mu[c], inv[c], clip) : 0.0f;
    }
};

struct SctCols {                                                  // stage 1 of mi_prep_sct_select: z = (float) the clipped residual
    int h;
    const double *par, *lu;                                       // par: b0, b1, alpha, h entries each; lu: per cell
    double clip, l;
    __device__ void bind_row(size_t row) { l = lu[row]; }
    __device__ float operator()(int c, float x) const
    {
        return c < h ? (float)sct_residual(x, par[c], par[h + c], par[2 * (size_t)h + c], l, clip) : 0.0f;
    }
};

// The dense kernels: one thread per element of Z, one cell per blockIdx.y.
__global__ void __launch_bounds__(256) k_prep_select(const float *__restrict__ Y, int n, int g, const int32_t *__restrict__ genes,
                                                     int h, int ldz, const float *__restrict__ mu, const float *__restrict__ inv,
                                                     const uint8_t *__restrict__ flat, float clip, float *__restrict__ Z)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    const size_t row = blockIdx.y;
    if (c >= ldz) return;
    float z = 0.0f;
    if (c < h && !flat[c]) z = scaled_value(Y[row * g + genes[c]], mu[c], inv[c], clip);
    Z[row * ldz + c] = z;
}

__global__ void __launch_bounds__(256) k_sct_select(const float *__restrict__ X, int g, const int32_t *__restrict__ genes, int h,
                                                    int ldz, const double *__restrict__ par, const double *__restrict__ lu,
                                                    double clip, float *__restrict__ Z)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    const size_t row = blockIdx.y;
    if (c >= ldz) return;
    float z = 0.0f;
    if (c < h) z = (float)sct_residual(X[row * g + genes[c]], par[c], par[h + c], par[2 * (size_t)h + c], lu[row], clip);
    Z[row * ldz + c] = z;
}

// ---- the sparse handle: counts as CSR (indptr, indices, values) plus the transpose as a position map (csrc/mi_prep_csr.h) ----
// Every kernel below reproduces the order of additions of its dense counterpart above on the densified matrix, so the
// results are the same bits: a skipped zero of a SUM adds +0.0 to a non-negative accumulator; a zero of the centred and
// clipped modes adds its per-gene constant, computed by the same operations, at that row's place in the order.

// one wavefront per cell: lane `col & 63` adds the entry, columns ascending (k_prep_normalize's lane-strided order)
__global__ void __launch_bounds__(256) k_prep_csr_normalize(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                            const float *__restrict__ X, float *__restrict__ Y, int n, double scale)
{
    const int lane = threadIdx.x & 63;
    const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (row >= n) return;
    const int64_t e0 = indptr[row], e1 = indptr[row + 1];
    double t = 0.0;
    for (int64_t b = e0; b < e1; b += 64) {
        const int cnt = __builtin_amdgcn_readfirstlane((int)(e1 - b < 64 ? e1 - b : 64));
        const int c = lane < cnt ? indices[b + lane] : 0;
        const float x = lane < cnt ? X[b + lane] : 0.0f;
        for (int i = 0; i < cnt; ++i) {
            const int ci = __builtin_amdgcn_readlane(c, i);
            const float xi = readlane_f(x, i);
            if (lane == (ci & 63)) t += (double)xi;
        }
    }
    t = wave_sum_f64(t);
    for (int64_t e = e0 + lane; e < e1; e += 64) Y[e] = t > 0.0 ? (float)log1p((double)X[e] * scale / t) : 0.0f;
}

// the first entry of a column's row list [k, end) at or below row r0
__device__ __forceinline__ int64_t csc_first_entry(const int32_t *__restrict__ rows, int64_t k, int64_t end, int r0)
{
    while (k < end) {
        const int64_t mid = k + ((end - k) >> 1);
        if (rows[mid] < r0) k = mid + 1; else end = mid;
    }
    return k;
}

// k_prep_col_partial<ColMode<Term>> on the transpose: thread (tx, ty) owns gene j and the rows r = ty (mod 4) of the slice;
// `vals` is in the caller's order and reached through pos.  The walk is the term's: the stored entries of the slice
// (kWalkStored), or all its rows, adding the stored value's term or the gene's constant of a zero (kWalkZeroConstant).  This
// kernel keeps its own prologue, LDS join and arguments: written over ColSlice and a mode argument it measured 1.5 - 2.4 %
// slower at 70 000 x 65 536 (profiles/prep_refactor_ab.json).
template <typename Term>
__global__ void __launch_bounds__(256) k_prep_csc_col_partial(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rows,
                                                              const int32_t *__restrict__ pos, const float *__restrict__ vals,
                                                              int n, int g, const double *__restrict__ mean,
                                                              const double *__restrict__ sd, double clip,
                                                              double *__restrict__ psum, int32_t *__restrict__ pnnz)
{
    __shared__ double s_sum[4][64];
    __shared__ int32_t s_cnt[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + tx;
    const int r0 = blockIdx.y * kRowSlice, r1 = r0 + kRowSlice < n ? r0 + kRowSlice : n;
    double acc = 0.0;
    int32_t cnt = 0;
    if (j < g) {
        const int64_t end = colptr[j + 1];
        int64_t k = csc_first_entry(rows, colptr[j], end, r0);
        // the next stored row of this thread's row lane inside the slice, r1 when there is none
        auto seek = [&]() -> int {
            for (; k < end; ++k) {
                const int r = rows[k];
                if (r >= r1) break;
                if ((r & 3) == ty) return r;
            }
            return r1;
        };
        int nr = seek();
        if (Term::kWalk == kWalkStored) {
            while (nr < r1) {
                const float v = vals[pos[k]];
                acc += Term::term(v, 0.0, 1.0, clip);
                cnt += v != 0.0f;
                ++k;
                nr = seek();
            }
        } else {
            const double mj = mean[j], sj = Term::kUsesSd ? sd[j] : 1.0;
            const double zero = Term::term(0.0f, mj, sj != 0.0 ? sj : 1.0, clip);
            if (!Term::kUsesSd || sj != 0.0) {
                int r = r0 + ty;
                while (r < r1) {
                    for (; r < nr; r += 4) acc += zero;
                    if (r >= r1) break;
                    acc += Term::term(vals[pos[k]], mj, sj, clip);    // (r == nr: both are = ty mod 4)
                    r += 4;
                    ++k;
                    nr = seek();
                }
            }
        }
    }
    s_sum[ty][tx] = acc;
    s_cnt[ty][tx] = cnt;
    __syncthreads();
    if (ty == 0 && j < g) {
        const size_t o = (size_t)blockIdx.y * g + j;
        psum[o] = ((s_sum[0][tx] + s_sum[1][tx]) + s_sum[2][tx]) + s_sum[3][tx];
        if (Term::kCounts) pnnz[o] = s_cnt[0][tx] + s_cnt[1][tx] + s_cnt[2][tx] + s_cnt[3][tx];
    }
}

// the transposed kernel of a mode whose zeros depend on the row (kWalkEveryRow): every row of the slice is computed, a
// stored value's term or that of 0.0f, over ColSlice like the dense kernel
template <typename Mode>
__global__ void __launch_bounds__(256) k_prep_csc_row_partial(const int64_t *__restrict__ colptr, const int32_t *__restrict__ rows,
                                                              const int32_t *__restrict__ pos, const float *__restrict__ vals,
                                                              int n, Mode mode, double *__restrict__ psum)
{
    const ColSlice s(n);
    double acc = 0.0;
    if (s.j < mode.count) {
        const int j = mode.bind(s.j);
        const int64_t end = colptr[j + 1];
        int64_t k = csc_first_entry(rows, colptr[j], end, s.r0);
        for (int r = s.r0 + s.ty; r < s.r1; r += 4) {
            while (k < end && rows[k] < r) ++k;
            acc += mode(k < end && rows[k] == r ? vals[pos[k]] : 0.0f, r);
        }
    }
    s.store(mode, acc, 0, psum, nullptr);
}

// One workgroup per cell builds a row of `count` floats in LDS -- at(c, 0.0f) in every column first, then, past a barrier,
// at(c, x) over the columns of the cell's stored entries of chosen genes (a gene is stored at most once per cell and chosen
// at most once: no two lanes write one word) -- and stores it as out[c * stride].  gmap: gene -> column, -1 = not chosen.
template <typename At>
__device__ __forceinline__ void csr_row_scatter(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                const float *__restrict__ vals, const int32_t *__restrict__ gmap, size_t row,
                                                int count, const At &at, float *__restrict__ out, size_t stride)
{
    __shared__ float s_row[MI_PREP_MAX_FEATURES];
    for (int c = threadIdx.x; c < count; c += 256) s_row[c] = at(c, 0.0f);
    __syncthreads();
    const int64_t e1 = indptr[row + 1];
    for (int64_t e = indptr[row] + threadIdx.x; e < e1; e += 256) {
        const int c = gmap[indices[e]];
        if (c >= 0) s_row[c] = at(c, vals[e]);
    }
    __syncthreads();
    for (int c = threadIdx.x; c < count; c += 256) out[c * stride] = s_row[c];
}

// k_prep_select from CSR, the row stored coalesced
template <typename Cols>
__global__ void __launch_bounds__(256) k_prep_csr_select(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                         const float *__restrict__ vals, const int32_t *__restrict__ gmap,
                                                         int ldz, Cols cols, float *__restrict__ Z)
{
    const size_t row = blockIdx.x;
    cols.bind_row(row);
    csr_row_scatter(indptr, indices, vals, gmap, row, ldz, cols, Z + row * ldz, 1);
}

// tile s of the row-major list of the upper block triangle: row I holds the tiles J = I .. T - 1
__device__ __forceinline__ void tile_of(int s, int T, int &I, int &J)
{
    I = 0;
    while (s >= T - I) {
        s -= T - I;
        ++I;
    }
    J = I + s;
}

__global__ void __launch_bounds__(256, 2) k_prep_gram(const float *__restrict__ Z, int ldz, int n, int T, int chunk0,
                                                      float *__restrict__ P)
{
    __shared__ __attribute__((aligned(16))) float As[kKC][kTile];
    __shared__ __attribute__((aligned(16))) float Bs[kKC][kTile];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int I, J;
    tile_of((int)blockIdx.x, T, I, J);
    const bool diag = I == J;
    const int c0 = (chunk0 + (int)blockIdx.y) * kChunk, c1 = c0 + kChunk < n ? c0 + kChunk : n;
    const int steps = (c1 - c0 + kKC - 1) / kKC;
    const int wi = (wave & 1) * 64, wj = (wave >> 1) * 64;         // this wavefront's 64 x 64 corner: rows (block I), columns (block J)
    const bool idle = diag && wi > wj;                            // the lower-left corner of a diagonal tile is its mirror's
    const int half = lane >> 5, col = lane & 31;
    const int kk = tid >> 5, c4 = (tid & 31) * 4;
    const float *za = Z + (size_t)I * kTile + c4, *zb = Z + (size_t)J * kTile + c4;

    f32x4 ra[4], rb[4];
    auto gload = [&](int step) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int cell = c0 + step * kKC + kk + 8 * q;
            ra[q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            rb[q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (cell < c1) {
                ra[q] = *reinterpret_cast<const f32x4 *>(za + (size_t)cell * ldz);
                if (!diag) rb[q] = *reinterpret_cast<const f32x4 *>(zb + (size_t)cell * ldz);
            }
        }
    };
    f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = f32x16{0};
    const float(*Bp)[kTile] = diag ? As : Bs;

    gload(0);
    for (int step = 0; step < steps; ++step) {
        __syncthreads();                                          // the MFMAs of the step before have read their operands
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            *reinterpret_cast<f32x4 *>(&As[kk + 8 * q][c4]) = ra[q];
            if (!diag) *reinterpret_cast<f32x4 *>(&Bs[kk + 8 * q][c4]) = rb[q];
        }
        __syncthreads();
        if (step + 1 < steps) gload(step + 1);                    // in flight under the MFMAs below
        if (idle) continue;
#pragma unroll
        for (int j = 0; j < kKC / 2; ++j) {
            const float a0 = As[2 * j + half][wi + col], a1 = As[2 * j + half][wi + 32 + col];
            const float b0 = Bp[2 * j + half][wj + col], b1 = Bp[2 * j + half][wj + 32 + col];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    if (idle) return;
    float *tile = P + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (kTile * kTile);
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int row = wi + 32 * a + (q & 3) + 8 * (q >> 2) + 4 * half;
                tile[row * kTile + wj + 32 * b + col] = acc[a][b][q];
            }
}

// G (T * 128 square, fp64) += the `nb` chunk tiles of every upper-triangle tile, chunk after chunk; entry and mirror get one value
__global__ void __launch_bounds__(256) k_prep_gram_reduce(const float *__restrict__ P, int tiles, int nb, int T,
                                                          double *__restrict__ G)
{
    int I, J;
    tile_of((int)blockIdx.x, T, I, J);
    const size_t ldg = (size_t)T * kTile;
    for (int e = threadIdx.x; e < kTile * kTile; e += 256) {
        const int r = e >> 7, c = e & (kTile - 1);
        if (I == J && r > c) continue;
        const size_t gr = (size_t)I * kTile + r, gc = (size_t)J * kTile + c;
        double t = G[gr * ldg + gc];
        for (int b = 0; b < nb; ++b) t += (double)P[((size_t)b * tiles + blockIdx.x) * (kTile * kTile) + e];
        G[gr * ldg + gc] = t;
        G[gc * ldg + gr] = t;
    }
}

// V: ldz x 128, zero padded both ways; hk = h rounded up to kKC (<= ldz)
__global__ void __launch_bounds__(256) k_prep_project(const float *__restrict__ Z, int ldz, int n, int hk,
                                                      const float *__restrict__ V, int p, float *__restrict__ out)
{
    __shared__ float Zs[kProjCells][kKC + 1];
    __shared__ __attribute__((aligned(16))) float Vs[kKC][kProjCols];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = lane >> 5, col = lane & 31;
    const int cell0 = (int)blockIdx.x * kProjCells;
    const bool idle = wave * 32 >= p;                             // a column block past p
    const int steps = hk / kKC;

    f32x4 rz[2], rv[4];
    auto gload = [&](int step) {
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + 256 * q, cell = cell0 + (e >> 3);
            rz[q] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
            if (cell < n) rz[q] = *reinterpret_cast<const f32x4 *>(Z + (size_t)cell * ldz + step * kKC + (e & 7) * 4);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q;
            rv[q] = *reinterpret_cast<const f32x4 *>(V + (size_t)(step * kKC + (e >> 5)) * kProjCols + (e & 31) * 4);
        }
    };
    f32x16 acc[2] = {f32x16{0}, f32x16{0}};

    gload(0);
    for (int step = 0; step < steps; ++step) {
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int e = tid + 256 * q;
            float *d = &Zs[e >> 3][(e & 7) * 4];
            d[0] = rz[q].x; d[1] = rz[q].y; d[2] = rz[q].z; d[3] = rz[q].w;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int e = tid + 256 * q;
            *reinterpret_cast<f32x4 *>(&Vs[e >> 5][(e & 31) * 4]) = rv[q];
        }
        __syncthreads();
        if (step + 1 < steps) gload(step + 1);
        if (idle) continue;
#pragma unroll
        for (int j = 0; j < kKC / 2; ++j) {
            const int k = 2 * j + half;
            const float a0 = Zs[col][k], a1 = Zs[32 + col][k], b = Vs[k][wave * 32 + col];
            acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1], 0, 0, 0);
        }
    }
    const int c = wave * 32 + col;
    if (idle || c >= p) return;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int cell = cell0 + 32 * a + (q & 3) + 8 * (q >> 2) + 4 * half;
            if (cell < n) out[(size_t)cell * p + c] = acc[a][q];
        }
}

// ---- per-cell QC: nCount, nFeature and the count of a gene subset (mask: g bytes of 0 / 1, or null) -----------------------
// The total is k_prep_normalize's (the same lane-strided fp64 sum, the same butterfly), so n_count is bit for bit what the
// normaliser divides by; the subset is the same walk over the masked genes; the features are counted in integers.

__device__ __forceinline__ int wave_sum_i32(int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

__global__ void __launch_bounds__(256) k_prep_cell_qc(const float *__restrict__ X, const uint8_t *__restrict__ mask, int n, int g,
                                                      double *__restrict__ n_count, int32_t *__restrict__ n_feature,
                                                      double *__restrict__ subset)
{
    const int lane = threadIdx.x & 63;
    const size_t row = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= (size_t)n) return;
    const float *x = X + row * g;
    double t = 0.0, s = 0.0;
    int c = 0;
    for (int j = lane; j < g; j += 64) {
        const float v = x[j];
        t += (double)v;
        if (mask && mask[j]) s += (double)v;
        c += v != 0.0f;
    }
    t = wave_sum_f64(t);
    s = wave_sum_f64(s);
    c = wave_sum_i32(c);
    if (lane == 0) {
        n_count[row] = t;
        n_feature[row] = c;
        subset[row] = s;
    }
}

// the same from CSR, in k_prep_csr_normalize's order: lane `col & 63` adds the entry, columns ascending (a skipped zero of the
// dense walk adds +0.0 to a non-negative sum); a stored zero is no feature
__global__ void __launch_bounds__(256) k_prep_csr_cell_qc(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                          const float *__restrict__ X, const uint8_t *__restrict__ mask, int n,
                                                          double *__restrict__ n_count, int32_t *__restrict__ n_feature,
                                                          double *__restrict__ subset)
{
    const int lane = threadIdx.x & 63;
    const int row = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (row >= n) return;
    const int64_t e0 = indptr[row], e1 = indptr[row + 1];
    double t = 0.0, s = 0.0;
    int c = 0;
    for (int64_t b = e0; b < e1; b += 64) {
        const int cnt = __builtin_amdgcn_readfirstlane((int)(e1 - b < 64 ? e1 - b : 64));
        const int col = lane < cnt ? indices[b + lane] : 0;
        const float x = lane < cnt ? X[b + lane] : 0.0f;
        const int in = lane < cnt && mask ? (int)mask[col] : 0;
        for (int i = 0; i < cnt; ++i) {
            const int ci = __builtin_amdgcn_readlane(col, i);
            const float xi = readlane_f(x, i);
            const int mi = __builtin_amdgcn_readlane(in, i);
            if (lane == (ci & 63)) {
                t += (double)xi;
                if (mi) s += (double)xi;
                c += xi != 0.0f;
            }
        }
    }
    t = wave_sum_f64(t);
    s = wave_sum_f64(s);
    c = wave_sum_i32(c);
    if (lane == 0) {
        n_count[row] = t;
        n_feature[row] = c;
        subset[row] = s;
    }
}

// ---- regression of covariates out of the gathered columns (mi_prep_select_regressed) --------------------------------------
// Z holds the h chosen columns of Y, unscaled.  The residuals' moments are k_prep_col_partial<RegressMoment>; the two kernels
// below stand on the same slices and lanes.  They read Z alone, so a sparse handle gives the bits of a dense one.

// psum[(slice * (q + 1) + k) * h + j]: k < q: sum_i Q_ik y_ij; k = q: sum_i y_ij^2
__global__ void __launch_bounds__(256) k_prep_regress_coef(const float *__restrict__ Z, int n, int h, int ldz,
                                                           const double *__restrict__ Q, int q, double *__restrict__ psum)
{
    const ColSlice s(n);
    double acc[kMaxQ + 1];
#pragma unroll
    for (int k = 0; k <= kMaxQ; ++k) acc[k] = 0.0;
    if (s.j < h) {
        for (int r = s.r0 + s.ty; r < s.r1; r += 4) {
            const double y = (double)Z[(size_t)r * ldz + s.j];
            const double *qr = Q + (size_t)r * q;
#pragma unroll
            for (int k = 0; k < kMaxQ; ++k)
                if (k < q) acc[k] += qr[k] * y;
            acc[kMaxQ] += y * y;
        }
    }
#pragma unroll
    for (int k = 0; k <= kMaxQ; ++k) {
        if (k >= q && k < kMaxQ) continue;                        // (uniform)
        s.join(acc[k], s.j < h, psum + ((size_t)blockIdx.y * (q + 1) + (k < q ? k : q)) * h + s.j);
        __syncthreads();                                          // (the next sum goes into the same words)
    }
}

// in place: z = flat ? 0 : (float) fmin((r - mean) * inv, clip), fp64 with one rounding to f32 (the padding columns keep
// the zeros of the gather)
__global__ void __launch_bounds__(256) k_prep_regress_scale(float *__restrict__ Z, int n, int h, int ldz, RegressColumn col,
                                                            const double *__restrict__ mean, const double *__restrict__ inv,
                                                            const uint8_t *__restrict__ flat, double clip)
{
    const ColSlice s(n);
    if (s.j >= h) return;
    col.bind(s.j, h);
    const double mj = mean[s.j], ij = inv[s.j];
    const bool fj = flat[s.j] != 0;
    for (int r = s.r0 + s.ty; r < s.r1; r += 4) {
        float *z = Z + (size_t)r * ldz + s.j;
        *z = fj ? 0.0f : (float)fmin((col.residual(*z, r) - mj) * ij, clip);
    }
}

// ---- SCTransform: negative-binomial regression on sequencing depth and Pearson residuals (include/mi_prep.h) -----------------
// The fit reads a dense f32 block of the counts (fit genes x fit cells, gene-major), written by one of two gathers, so it
// never sees the handle's kind: a sparse handle gives the bits of a dense one.
constexpr int kFitCells = MI_PREP_SCT_MAX_FIT_CELLS;
constexpr int kFitPoissonSteps = 8, kFitRounds = 40;
constexpr double kFitTol = 1e-16;

// B[jj * mc + ii] = X[cells[ii], genes[jj]]: one thread per element
__global__ void __launch_bounds__(256) k_sct_gather(const float *__restrict__ X, int g, const int32_t *__restrict__ cells, int mc,
                                                    const int32_t *__restrict__ genes, int g1, float *__restrict__ B)
{
    const int jj = blockIdx.x * 256 + threadIdx.x, ii = blockIdx.y;
    if (jj >= g1) return;
    B[(size_t)jj * mc + ii] = X[(size_t)cells[ii] * g + genes[jj]];
}

// the same from CSR: one workgroup per fit cell scatters its row of the block (the counts as they are) and stores it gene-major
__global__ void __launch_bounds__(256) k_sct_csr_gather(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                        const float *__restrict__ X, const int32_t *__restrict__ gmap,
                                                        const int32_t *__restrict__ cells, int mc, int g1, float *__restrict__ B)
{
    const int ii = blockIdx.x;
    csr_row_scatter(indptr, indices, X, gmap, (size_t)cells[ii], g1, [](int, float x) { return x; }, B + ii, (size_t)mc);
}

// K sums of a workgroup of 256: the wave butterfly, then the four waves in LDS as ((s0 + s1) + s2) + s3; every thread
// leaves with the same bits, so the scalar logic that follows is workgroup-uniform
template <int K>
__device__ __forceinline__ void fit_block_sum(double (&v)[K], double (*s_red)[4])
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum_f64(v[k]);
    __syncthreads();                                              // (the readers of the previous sums are through)
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) s_red[k][w] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = ((s_red[k][0] + s_red[k][1]) + s_red[k][2]) + s_red[k][3];
}

// One workgroup per gene: y ~ NB(mu, alpha), log mu = b0 + b1 xc.  The gene's counts sit in LDS (<= kFitCells floats), xc is
// shared by all genes (fp64, L2), mu is recomputed in every pass: nothing per cell is kept between rounds.  Thread t adds the
// cells t, t + 256, ... ascending.  The algorithm, step by step: include/mi_prep.h (mi_prep_nb_fit).
__global__ void __launch_bounds__(256) k_sct_nb_fit(const float *__restrict__ B, int mc, const double *__restrict__ xc, double xmean,
                                                    double *__restrict__ o_b0, double *__restrict__ o_b1,
                                                    double *__restrict__ o_alpha, double *__restrict__ o_se_b0c,
                                                    double *__restrict__ o_se_b1, double *__restrict__ o_se_alpha,
                                                    int32_t *__restrict__ o_iter, uint8_t *__restrict__ o_conv,
                                                    uint8_t *__restrict__ o_pois)
{
    __shared__ float s_y[kFitCells];
    __shared__ double s_red[5][4];
    const int j = blockIdx.x, t = threadIdx.x;
    for (int i = t; i < mc; i += 256) s_y[i] = B[(size_t)j * mc + i];
    __syncthreads();
    double b0 = 0.0, b1 = 0.0;
    // 1. the Poisson start: IRLS from mu = y + 0.1, each step the closed form of the 2 x 2 weighted normal equations
    for (int it = 0; it < kFitPoissonSteps; ++it) {
        double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = t; i < mc; i += 256) {
            const double y = (double)s_y[i], x = xc[i];
            double mu, eta;
            if (it == 0) {
                mu = y + 0.1;
                eta = log(mu);
            } else {
                eta = b0 + b1 * x;
                mu = exp(eta);
            }
            const double z = eta + (y - mu) / mu, wx = mu * x;
            a[0] += mu;
            a[1] += wx;
            a[2] += wx * x;
            a[3] += mu * z;
            a[4] += wx * z;
        }
        fit_block_sum<5>(a, s_red);
        const double det = a[0] * a[2] - a[1] * a[1];
        b0 = (a[2] * a[3] - a[1] * a[4]) / det;
        b1 = (a[0] * a[4] - a[1] * a[3]) / det;
    }
    // 2. the Poisson rule, once, at the Poisson fit
    double alpha;
    bool pois;
    {
        double a[2] = {0.0, 0.0};
        for (int i = t; i < mc; i += 256) {
            const double y = (double)s_y[i], mu = exp(b0 + b1 * xc[i]), d = y - mu;
            a[0] += d * d - y;
            a[1] += mu * mu;
        }
        fit_block_sum<2>(a, s_red);
        pois = !(a[0] > 0.0);
        alpha = pois ? 0.0 : a[0] / a[1];
    }
    // 3. the rounds
    int iters = 0;
    bool conv = false;
    double l2 = 0.0, i00 = 0.0, i11 = 0.0, det = 0.0;
    for (int round = 0; round < kFitRounds && !conv; ++round) {
        double l1 = 0.0, anew = alpha;
        if (!pois) {
            const double th = 1.0 / alpha, psi0 = mi_sct::digamma(th), tri0 = mi_sct::trigamma(th);
            double a[2] = {0.0, 0.0};
            for (int i = t; i < mc; i += 256) {
                const double y = (double)s_y[i], mu = exp(b0 + b1 * xc[i]);
                const double tm = th + mu, d = y - mu;
                double dpsi = 0.0, dtri = 0.0;                    // (psi(th) - psi(th) is +0.0: a zero count skips both)
                if (y != 0.0) {
                    dpsi = mi_sct::digamma(y + th) - psi0;
                    dtri = mi_sct::trigamma(y + th) - tri0;
                }
                a[0] += (dpsi + log1p(-(mu / tm))) - d / tm;
                a[1] += (dtri + mu / (th * tm)) + d / (tm * tm);
            }
            fit_block_sum<2>(a, s_red);
            const double th2 = th * th;
            l1 = -(th2 * a[0]);
            l2 = (th2 * th2) * a[1] + 2.0 * ((th2 * th) * a[0]);
            if (l2 < 0.0)
                anew = alpha - l1 / l2;
            else
                anew = l1 > 0.0 ? 2.0 * alpha : 0.5 * alpha;
            if (!(anew > 0.0)) anew = 0.25 * alpha;
            anew = fmin(fmax(anew, 0.125 * alpha), 8.0 * alpha);
        }
        double a[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
        for (int i = t; i < mc; i += 256) {
            const double y = (double)s_y[i], x = xc[i], mu = exp(b0 + b1 * x);
            const double den = 1.0 + anew * mu, w = mu / den, u = (y - mu) / den, wx = w * x;
            a[0] += u;
            a[1] += u * x;
            a[2] += w;
            a[3] += wx;
            a[4] += wx * x;
        }
        fit_block_sum<5>(a, s_red);
        det = a[2] * a[4] - a[3] * a[3];
        i00 = a[2];
        i11 = a[4];
        const double d0 = (a[4] * a[0] - a[3] * a[1]) / det, d1 = (a[2] * a[1] - a[3] * a[0]) / det;
        double lam2 = a[0] * d0 + a[1] * d1;
        if (!pois) lam2 = l2 < 0.0 ? lam2 + (l1 * l1) / -l2 : HUGE_VAL;
        b0 = b0 + d0;
        b1 = b1 + d1;
        alpha = anew;
        ++iters;
        conv = lam2 <= kFitTol;
    }
    if (t == 0) {
        o_b0[j] = b0 - b1 * xmean;
        o_b1[j] = b1;
        o_alpha[j] = alpha;
        o_se_b0c[j] = sqrt(i11 / det);
        o_se_b1[j] = sqrt(i00 / det);
        o_se_alpha[j] = !pois && l2 < 0.0 ? 1.0 / sqrt(-l2) : __builtin_nan("");
        o_iter[j] = iters;
        o_conv[j] = conv;
        o_pois[j] = pois;
    }
}

// ---- SCTransform's corrected counts (mi_prep_sct_correct): a second matrix from (counts, regularised model) ------------------
// c = mi_sct::corrected_count(x, exp(b0 + b1 log_umi_i), alpha, mu_r, s_r) and the data slot (float) log1p(c).  The table
// `tab` holds, per gene of the handle, b0, b1, alpha and the two values at the reference depth, mu_r and s_r, computed once
// per gene (5 rows of g); listed[j] = 0 marks a gene that is not listed, whose column is all zero.  Every kernel below
// evaluates through SctGene alone, on the stored value or on 0.0f for a zero, so the sparse form gives the dense form's bits.
// A sparse result has its own structure: the row pass (k_sct_csr_rows: count, k_prep_scan_counts, fill) builds its CSR in
// order, and its transpose is a counting sort of that CSR (k_csr_block_*), which evaluates nothing.
constexpr int kCorrChunk = 4096;                                  // genes of a cell (cells of a gene) in LDS at a time: 32 KB of fp64

__global__ void __launch_bounds__(256) k_sct_gene_table(const int32_t *__restrict__ genes, const double *__restrict__ par, int gp,
                                                        double lu_ref, int g, double *__restrict__ tab,
                                                        uint8_t *__restrict__ listed)
{
    const int jj = blockIdx.x * 256 + threadIdx.x;
    if (jj >= gp) return;
    const size_t j = (size_t)genes[jj], gs = (size_t)g;
    const double b0 = par[jj], b1 = par[gp + jj], al = par[2 * (size_t)gp + jj];
    const double mur = exp(b0 + b1 * lu_ref);
    tab[j] = b0;
    tab[gs + j] = b1;
    tab[2 * gs + j] = al;
    tab[3 * gs + j] = mur;
    tab[4 * gs + j] = mi_sct::nb_sd(mur, al);
    listed[j] = 1;
}

struct SctGene {                                                  // one gene's column of the table
    double b0, b1, al, mur, sr;
    __device__ __forceinline__ SctGene(const double *__restrict__ tab, int g, int j)
        : b0(tab[j]), b1(tab[(size_t)g + j]), al(tab[2 * (size_t)g + j]), mur(tab[3 * (size_t)g + j]), sr(tab[4 * (size_t)g + j])
    {
    }
    // the corrected count of x in a cell of log_umi l; a value that is not finite raises *bad (every writer stores 1)
    __device__ __forceinline__ double operator()(float x, double l, int *__restrict__ bad) const
    {
        bool finite;
        const double c = mi_sct::corrected_count((double)x, exp(b0 + b1 * l), al, mur, sr, &finite);
        if (!finite) *bad = 1;
        return c;
    }
};

// the dense form, on the slices and lanes of k_prep_col_partial (a thread keeps its gene's column of the table over its rows):
// C = (float) c and D = (float) log1p(c), n x g each
__global__ void __launch_bounds__(256) k_sct_correct(const float *__restrict__ X, int n, int g, const double *__restrict__ tab,
                                                     const uint8_t *__restrict__ listed, const double *__restrict__ lu,
                                                     float *__restrict__ Cm, float *__restrict__ Dm, int *__restrict__ bad)
{
    const ColSlice s(n);
    if (s.j >= g) return;
    const bool on = listed[s.j] != 0;
    const SctGene gene(tab, g, on ? s.j : 0);
    for (int r = s.r0 + s.ty; r < s.r1; r += 4) {
        const size_t e = (size_t)r * g + s.j;
        const double c = on ? gene(X[e], lu[r], bad) : 0.0;
        Cm[e] = (float)c;
        Dm[e] = (float)log1p(c);
    }
}

__device__ __forceinline__ int lanes_below(unsigned long long mask)
{
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// the sum of v over the workgroup of 256 (integers: any order gives the same value), in every thread
__device__ __forceinline__ int block_sum_i32(int v, int *s_w)
{
    v = wave_sum_i32(v);
    if ((threadIdx.x & 63) == 0) s_w[threadIdx.x >> 6] = v;
    __syncthreads();
    return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}

// Ordered compaction of a chunk in LDS: emit(i, o) for every i < len with s[i] != 0, o counting up from `base` in ascending
// i.  Wavefront w owns the quarter [w kCorrChunk / 4, ...): it counts its non-zeros by ballots, the four counts meet in LDS,
// and it walks its quarter again with the prefix of the wavefronts before it; inside a ballot the place is the count of
// the lanes below.  -> base + the chunk's non-zeros.  Ends on a barrier: s and s_w are free again.
template <typename Emit>
__device__ __forceinline__ int64_t chunk_compact(const double *s, int len, int64_t base, int *s_w, const Emit &emit)
{
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int i0 = w * (kCorrChunk / 4), i1 = i0 + kCorrChunk / 4 < len ? i0 + kCorrChunk / 4 : len;
    int cnt = 0;
    for (int i = i0; i < i1; i += 64) cnt += __popcll(__ballot(i + lane < i1 && s[i + lane] != 0.0));
    if (lane == 0) s_w[w] = cnt;
    __syncthreads();
    int64_t o = base;
    for (int k = 0; k < w; ++k) o += s_w[k];
    const int total = s_w[0] + s_w[1] + s_w[2] + s_w[3];
    for (int i = i0; i < i1; i += 64) {
        const bool nz = i + lane < i1 && s[i + lane] != 0.0;
        const unsigned long long b = __ballot(nz);
        if (nz) emit(i + lane, o + lanes_below(b));
        o += __popcll(b);
    }
    __syncthreads();
    return base + total;
}

// The row pass of the sparse form, one workgroup per cell: by chunk of genes the zeros' corrected counts fill the cell's LDS
// row, the stored entries of listed genes overwrite theirs (a gene is stored at most once per cell).  PASS 0 counts the
// non-zeros of the row; PASS 1, given the scanned counts as new_indptr, evaluates again and writes columns (ascending), counts
// and data slot.
template <int PASS>
__global__ void __launch_bounds__(256) k_sct_csr_rows(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                      const float *__restrict__ X, int g, const double *__restrict__ tab,
                                                      const uint8_t *__restrict__ listed, const double *__restrict__ lu,
                                                      int32_t *__restrict__ row_count, const int64_t *__restrict__ new_indptr,
                                                      int32_t *__restrict__ new_indices, float *__restrict__ Cv,
                                                      float *__restrict__ Dv, int *__restrict__ bad)
{
    __shared__ double s_c[kCorrChunk];
    __shared__ int s_w[4];
    const size_t row = blockIdx.x;
    const double l = lu[row];
    const int64_t e0 = indptr[row], e1 = indptr[row + 1];
    int64_t out = PASS ? new_indptr[row] : 0;
    const int64_t end = PASS ? new_indptr[row + 1] : 0;          // (the count pass gave this row's room: nothing is written past it)
    int cnt = 0;
    for (int c0 = 0; c0 < g; c0 += kCorrChunk) {
        const int len = g - c0 < kCorrChunk ? g - c0 : kCorrChunk;
        for (int i = threadIdx.x; i < len; i += 256) s_c[i] = listed[c0 + i] ? SctGene(tab, g, c0 + i)(0.0f, l, bad) : 0.0;
        __syncthreads();
        const int64_t a = csc_first_entry(indices, e0, e1, c0), b = csc_first_entry(indices, a, e1, c0 + len);
        for (int64_t e = a + threadIdx.x; e < b; e += 256) {
            const int j = indices[e];
            if (listed[j]) s_c[j - c0] = SctGene(tab, g, j)(X[e], l, bad);
        }
        __syncthreads();
        if (PASS == 0) {
            for (int i = threadIdx.x; i < len; i += 256) cnt += s_c[i] != 0.0;
            __syncthreads();
        } else {
            out = chunk_compact(s_c, len, out, s_w, [&](int i, int64_t o) {
                const double c = s_c[i];
                if (o >= end) return;
                new_indices[o] = c0 + i;
                Cv[o] = (float)c;
                Dv[o] = (float)log1p(c);
            });
        }
    }
    if (PASS == 0) {
        cnt = block_sum_i32(cnt, s_w);
        if (threadIdx.x == 0) row_count[row] = cnt;
    }
}

// The transpose of a CSR structure built on the device, by a two-level counting sort that evaluates nothing: the rows are cut
// into blocks of R, hist[b g + j] counts the entries of gene j in block b (integer atomics: any order gives the same
// counts), k_csr_block_offsets turns each gene's counts into the exclusive prefix over the blocks (and the gene's total),
// and k_csr_block_transpose, one workgroup per block, walks its rows one after another -- a row's columns are distinct, so
// its entries take their places side by side; a barrier parts the rows -- which leaves every gene's cells ascending.
__global__ void __launch_bounds__(256) k_csr_block_hist(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                        int n, int g, int R, int32_t *__restrict__ hist)
{
    const int r0 = blockIdx.x * R, r1 = r0 + R < n ? r0 + R : n;
    int32_t *h = hist + (size_t)blockIdx.x * g;
    const int64_t e1 = indptr[r1];
    for (int64_t e = indptr[r0] + threadIdx.x; e < e1; e += 256) atomicAdd(&h[indices[e]], 1);
}

__global__ void __launch_bounds__(256) k_csr_block_offsets(int32_t *__restrict__ hist, int nb, int g, int32_t *__restrict__ count)
{
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= g) return;
    int32_t run = 0;
    for (int b = 0; b < nb; ++b) {
        const size_t o = (size_t)b * g + j;
        const int32_t c = hist[o];
        hist[o] = run;
        run += c;
    }
    count[j] = run;
}

__global__ void __launch_bounds__(256) k_csr_block_transpose(const int64_t *__restrict__ indptr, const int32_t *__restrict__ indices,
                                                             int n, int g, int R, const int64_t *__restrict__ colptr,
                                                             int32_t *hist, int32_t *__restrict__ rows, int32_t *__restrict__ pos)
{
    const int r0 = blockIdx.x * R, r1 = r0 + R < n ? r0 + R : n;
    int32_t *h = hist + (size_t)blockIdx.x * g;
    for (int r = r0; r < r1; ++r) {
        const int64_t e1 = indptr[r + 1];
        for (int64_t e = indptr[r] + threadIdx.x; e < e1; e += 256) {
            const int j = indices[e];
            const int32_t k = h[j];
            h[j] = k + 1;
            const int64_t o = colptr[j] + k;
            rows[o] = r;
            pos[o] = (int32_t)e;
        }
        __syncthreads();                                          // (the next row reads the cursors this one moved)
    }
}

// out[0] = 0, out[i + 1] = in[0] + ... + in[i] in 64 bits.  One workgroup, 1024 counts at a time: an inclusive scan inside
// each wavefront by shuffles, the sixteen totals through LDS, the tiles before as a carry every thread keeps.
__global__ void __launch_bounds__(1024) k_prep_scan_counts(const int32_t *__restrict__ in, int64_t *__restrict__ out, int n)
{
    __shared__ long long s_w[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long carry = 0;
    if (threadIdx.x == 0) out[0] = 0;
    for (int base = 0; base < n; base += 1024) {
        const int i = base + (int)threadIdx.x;
        long long v = i < n ? (long long)in[i] : 0;
        for (int off = 1; off < 64; off <<= 1) {
            const long long u = __shfl_up(v, off, 64);
            if (lane >= off) v += u;
        }
        if (lane == 63) s_w[w] = v;
        __syncthreads();
        long long before = carry;
        for (int k = 0; k < 16; ++k) {
            if (k < w) before += s_w[k];
            carry += s_w[k];
        }
        if (i < n) out[i + 1] = before + v;
        __syncthreads();
    }
}

}  // namespace
}  // namespace mi_sa_impl
using namespace mi_sa_impl;

// (mi_prep_matrix and on_matrix, the way into every entry below: mi_prep_handle.h)

namespace {

int slices(const mi_prep_matrix *m) { return (m->n + kRowSlice - 1) / kRowSlice; }

// out[e] = (sum over the slices, ascending, of psum[slice * count + e]) / denom; with d_pnnz, out_nnz[e] = the counts' sum
int finish_slices(const double *d_psum, const int32_t *d_pnnz, int nslices, size_t count, double denom, double *d_out,
                  int32_t *d_out_nnz)
{
    hipLaunchKernelGGL(k_prep_col_finish, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, 0, d_psum, d_pnnz, nslices,
                       (int)count, denom, d_out, d_out_nnz);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// the partials of `mode` per slice of the dense M (n x ld)
template <typename Mode>
int col_partials_dense(const float *M, int ld, int n, const Mode &mode, double *d_psum, int32_t *d_pnnz)
{
    const dim3 grid((unsigned)((mode.count + 63) / 64), (unsigned)((n + kRowSlice - 1) / kRowSlice));
    hipLaunchKernelGGL(k_prep_col_partial<Mode>, grid, dim3(256), 0, 0, M, ld, n, mode, d_psum, d_pnnz);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

// One column reduction over M, the handle's counts or normalised values: the partials by the kernel of the handle's kind,
// then the ordered sum divided by denom (device pointers in and out; d_pnnz and d_out_nnz: the modes that count).
template <typename Mode>
int col_reduce(const mi_prep_matrix *m, const float *M, const Mode &mode, double denom, double *d_psum, int32_t *d_pnnz,
               double *d_out, int32_t *d_out_nnz)
{
    if (m->sparse) {
        const dim3 grid((unsigned)((mode.count + 63) / 64), (unsigned)slices(m));
        if constexpr (Mode::kWalk == kWalkEveryRow)
            hipLaunchKernelGGL(k_prep_csc_row_partial<Mode>, grid, dim3(256), 0, 0, m->d_colptr, m->d_rows, m->d_pos, M, m->n, mode,
                               d_psum);
        else
            hipLaunchKernelGGL(k_prep_csc_col_partial<typename Mode::Term>, grid, dim3(256), 0, 0, m->d_colptr, m->d_rows,
                               m->d_pos, M, m->n, mode.count, mode.mean, mode.sd, mode.clip, d_psum, d_pnnz);
        HIP_TRY(hipGetLastError());
    } else {
        MI_TRY(col_partials_dense(M, m->g, m->n, mode, d_psum, d_pnnz));
    }
    return finish_slices(d_psum, Mode::kCounts ? d_pnnz : nullptr, slices(m), (size_t)mode.count, denom, d_out, d_out_nnz);
}

// Z sized for h columns (ldz: h rounded up to the Gram tile); a failure leaves it empty
int size_Z(mi_prep_matrix *m, int h)
{
    const int ldz = (h + kTile - 1) / kTile * kTile;
    HIP_TRY(m->d_Z.resize((size_t)m->n * ldz));
    m->ldz = ldz;
    return MI_OK;
}

// one slab of the dense selection: `rows` cells from cell r0 on, M and Z already at that cell
void launch_dense_select(dim3 grid, const float *M, int rows, int g, const int32_t *d_genes, int ldz, const ScaledCols &c, int,
                         float *Z)
{
    hipLaunchKernelGGL(k_prep_select, grid, dim3(256), 0, 0, M, rows, g, d_genes, c.h, ldz, c.mu, c.inv, c.flat, c.clip, Z);
}

void launch_dense_select(dim3 grid, const float *M, int, int g, const int32_t *d_genes, int ldz, const SctCols &c, int r0, float *Z)
{
    hipLaunchKernelGGL(k_sct_select, grid, dim3(256), 0, 0, M, g, d_genes, c.h, ldz, c.par, c.lu + r0, c.clip, Z);
}

// Z (n x ldz) = `cols` of the chosen columns of M, by the select kernel of the handle's kind (device pointers; d_gmap: sparse only)
template <typename Cols>
int launch_select(const mi_prep_matrix *m, const float *M, const int32_t *d_genes, const int32_t *d_gmap, const Cols &cols)
{
    const int ldz = m->ldz;
    if (m->sparse) {
        hipLaunchKernelGGL(k_prep_csr_select<Cols>, dim3((unsigned)m->n), dim3(256), 0, 0, m->d_indptr, m->d_indices, M, d_gmap,
                           ldz, cols, m->d_Z);
        HIP_TRY(hipGetLastError());
        return MI_OK;
    }
    for (int r0 = 0; r0 < m->n; r0 += 32768) {                    // (one cell per grid.y, whose limit is 65535: slabs of 32768 cells)
        const int rows = m->n - r0 < 32768 ? m->n - r0 : 32768;
        launch_dense_select(dim3((unsigned)(ldz / 256 + (ldz % 256 != 0)), (unsigned)rows), M + (size_t)r0 * m->g, rows, m->g,
                            d_genes, ldz, cols, r0, m->d_Z + (size_t)r0 * ldz);
        HIP_TRY(hipGetLastError());
    }
    return MI_OK;
}

// stages 2 - 5 of mi_prep_select_regressed on the gathered Z (n x ldz, h columns): c = Q^T y and S, the residuals' mean and
// squares, the flat rule and 1 / sd in host fp64 (unit_scale: 1 in place of 1 / sd), the scaling in place.  d_Q: device.
int regress_stages(mi_prep_matrix *m, int h, const double *d_Q, int q, double clip, bool unit_scale, double *out_coef,
                   double *out_mean, double *out_var, uint8_t *out_flat, float *out_ms)
{
    const size_t hs = (size_t)h, qs = (size_t)q;
    const int ldz = m->ldz, ns = slices(m);
    std::vector<uint8_t> flat(hs, 0);
    std::vector<double> S(hs), ss(hs), inv(hs), var(hs);
    DevBufs bufs;
    uint8_t *d_flat;
    double *d_psum, *d_coef, *d_mean, *d_ss, *d_inv;
    HIP_TRY(bufs.alloc(&d_psum, (size_t)ns * (qs + 1) * hs));
    HIP_TRY(bufs.alloc(&d_coef, (qs + 1) * hs));                  // q rows of coefficients, then S
    HIP_TRY(bufs.alloc(&d_mean, hs));
    HIP_TRY(bufs.alloc(&d_ss, hs));
    const RegressColumn col{d_Q, q, d_coef};
    float ms1 = 0.0f, ms2 = 0.0f;
    {
        Timer t;
        MI_TRY(t.start(0));
        // 2. c = Q^T y and S = sum y^2
        hipLaunchKernelGGL(k_prep_regress_coef, dim3((unsigned)((h + 63) / 64), (unsigned)ns), dim3(256), 0, 0, m->d_Z, m->n, h,
                           ldz, d_Q, q, d_psum);
        HIP_TRY(hipGetLastError());
        MI_TRY(finish_slices(d_psum, nullptr, ns, (qs + 1) * hs, 1.0, d_coef, nullptr));
        // 3. the mean of the residuals, then their squares about it
        MI_TRY(col_partials_dense(m->d_Z, ldz, m->n, RegressMoment<0>{h, col, nullptr}, d_psum, nullptr));
        MI_TRY(finish_slices(d_psum, nullptr, ns, hs, (double)m->n, d_mean, nullptr));
        MI_TRY(col_partials_dense(m->d_Z, ldz, m->n, RegressMoment<1>{h, col, d_mean}, d_psum, nullptr));
        MI_TRY(finish_slices(d_psum, nullptr, ns, hs, 1.0, d_ss, nullptr));
        MI_TRY(t.stop(0, &ms1));
    }
    // 4. the flat rule and the inverse standard deviation, in host fp64
    HIP_TRY(hipMemcpy(S.data(), d_coef + qs * hs, hs * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(ss.data(), d_ss, hs * sizeof(double), hipMemcpyDeviceToHost));
    for (int c = 0; c < h; ++c) {
        var[c] = ss[c] / (double)(m->n - 1);
        flat[c] = ss[c] <= 1e-16 * S[c];
        inv[c] = flat[c] ? 0.0 : (unit_scale ? 1.0 : 1.0 / std::sqrt(var[c]));
    }
    HIP_TRY(bufs.upload(&d_flat, flat.data(), hs));
    HIP_TRY(bufs.upload(&d_inv, inv.data(), hs));
    {
        Timer t;
        MI_TRY(t.start(0));
        // 5. scale in place
        hipLaunchKernelGGL(k_prep_regress_scale, dim3((unsigned)((h + 63) / 64), (unsigned)ns), dim3(256), 0, 0, m->d_Z, m->n, h,
                           ldz, col, d_mean, d_inv, d_flat, clip);
        MI_TRY(t.stop(0, &ms2));
    }
    if (out_ms) *out_ms = ms1 + ms2;
    if (out_coef) HIP_TRY(hipMemcpy(out_coef, d_coef, qs * hs * sizeof(double), hipMemcpyDeviceToHost));
    if (out_mean) HIP_TRY(hipMemcpy(out_mean, d_mean, hs * sizeof(double), hipMemcpyDeviceToHost));
    if (out_var) std::copy(var.begin(), var.end(), out_var);
    if (out_flat) std::copy(flat.begin(), flat.end(), out_flat);
    return MI_OK;
}

// MI_EINVAL unless the `count` indices are distinct and inside [0, limit); `what` names the array, `one` an element
int check_indices(const int32_t *idx, int count, int limit, const char *what, const char *one)
{
    std::vector<uint8_t> seen((size_t)limit, 0);
    for (int c = 0; c < count; ++c) {
        const int32_t j = idx[c];
        if (j < 0 || j >= limit) return fail(MI_EINVAL, "%s[%d] = %d is outside [0, %d)", what, c, (int)j, limit);
        if (seen[j]) return fail(MI_EINVAL, "%s %d is chosen twice", one, (int)j);
        seen[j] = 1;
    }
    return MI_OK;
}

// the map gene -> its place among the `count` chosen genes, -1 = not chosen (what the CSR kernels scatter through)
std::vector<int32_t> gene_map(const mi_prep_matrix *m, const int32_t *genes, int count)
{
    std::vector<int32_t> gmap((size_t)m->g, -1);
    for (int c = 0; c < count; ++c) gmap[genes[c]] = c;
    return gmap;
}

// the chosen genes on the device and, for a sparse handle, their gene_map (null for a dense one)
int upload_genes(DevBufs &bufs, const mi_prep_matrix *m, const int32_t *genes, int count, int32_t **d_genes, int32_t **d_gmap)
{
    HIP_TRY(bufs.upload(d_genes, genes, (size_t)count));
    *d_gmap = nullptr;
    if (m->sparse) {
        const std::vector<int32_t> gmap = gene_map(m, genes, count);
        HIP_TRY(bufs.upload(d_gmap, gmap.data(), gmap.size()));
    }
    return MI_OK;
}

// Q: n x q row-major
int check_Q(const double *Q, size_t n, size_t q)
{
    for (size_t e = 0; e < n * q; ++e)
        if (!std::isfinite(Q[e])) return fail(MI_EINVAL, "Q[%lld, %lld] is not finite", (long long)(e / q), (long long)(e % q));
    return MI_OK;
}

// the three parameter rows of the residual kernels (b0, b1, alpha: count entries each), checked, as one array
int pack_nb_parameters(const double *b0, const double *b1, const double *alpha, int count, std::vector<double> &par)
{
    par.resize(3 * (size_t)count);
    for (int c = 0; c < count; ++c) {
        if (!std::isfinite(b0[c]) || !std::isfinite(b1[c])) return fail(MI_EINVAL, "b0[%d] or b1[%d] is not finite", c, c);
        if (!(alpha[c] >= 0.0) || std::isinf(alpha[c])) return fail(MI_EINVAL, "alpha[%d] must be finite and >= 0", c);
        par[c] = b0[c];
        par[(size_t)count + c] = b1[c];
        par[2 * (size_t)count + c] = alpha[c];
    }
    return MI_OK;
}

int check_log_umi(const double *log_umi, int count)
{
    for (int i = 0; i < count; ++i)
        if (!std::isfinite(log_umi[i])) return fail(MI_EINVAL, "log_umi[%d] is not finite (a cell without counts?)", i);
    return MI_OK;
}

}  // namespace

extern "C" {

int mi_prep_destroy(mi_prep_matrix *m)
{
    if (!m) return MI_OK;
    (void)hipSetDevice(m->device);
    delete m;
    return MI_OK;
}

int mi_prep_create_f32(const float *X, int n, int g, int device, mi_prep_matrix **out)
{
    if (out) *out = nullptr;
    if (!X || !out) return fail(MI_EINVAL, "NULL argument");
    if (n < 2) return fail(MI_EINVAL, "n must be >= 2 (got %d)", n);
    if (g < 1) return fail(MI_EINVAL, "g must be >= 1 (got %d)", g);
    if (n > MI_PREP_MAX_CELLS) return fail(MI_EUNSUPPORTED, "%d cells exceed %d", n, MI_PREP_MAX_CELLS);
    if ((long long)n * g > MI_PREP_MAX_ENTRIES)
        return fail(MI_EUNSUPPORTED, "%d x %d entries exceed %lld", n, g, (long long)MI_PREP_MAX_ENTRIES);
    const size_t cells = (size_t)n * g;
    for (size_t e = 0; e < cells; ++e)
        if (!(X[e] >= 0.0f) || std::isinf(X[e]))
            return fail(MI_EINVAL, "X[%lld, %lld] is NaN, infinite or negative", (long long)(e / g), (long long)(e % g));
    return guarded([&]() -> int {
        MI_TRY(pick_device(device));
        mi_prep_matrix *m = new mi_prep_matrix();
        m->n = n; m->g = g; m->device = device;
        const int rc = [&]() -> int {
            HIP_TRY(m->d_X.upload(X, cells));
            return MI_OK;
        }();
        if (rc != MI_OK) {
            mi_prep_destroy(m);
            return rc;
        }
        *out = m;
        return MI_OK;
    });
}

int mi_prep_create_csr_f32(const int64_t *indptr, const int32_t *indices, const float *data, int n, int g, int device,
                           mi_prep_matrix **out)
{
    if (out) *out = nullptr;
    if (!out) return fail(MI_EINVAL, "NULL argument");
    char msg[160];
    const int bad = mi_prep_csr::check(indptr, indices, data, n, g, MI_PREP_MAX_CELLS, MI_PREP_MAX_NNZ, msg, sizeof msg);
    if (bad != mi_prep_csr::kOk) return fail(bad == mi_prep_csr::kEinval ? MI_EINVAL : MI_EUNSUPPORTED, "%s", msg);
    return guarded([&]() -> int {
        std::vector<int64_t> colptr;
        std::vector<int32_t> rows, pos;
        mi_prep_csr::transpose(indptr, indices, n, g, colptr, rows, pos);
        MI_TRY(pick_device(device));
        mi_prep_matrix *m = new mi_prep_matrix();
        m->n = n; m->g = g; m->device = device; m->sparse = true; m->nnz = indptr[n];
        const size_t nnz = (size_t)m->nnz;
        const int rc = [&]() -> int {
            HIP_TRY(m->d_indptr.upload(indptr, (size_t)n + 1));
            HIP_TRY(m->d_indices.upload(indices, nnz));
            HIP_TRY(m->d_X.upload(data, nnz));
            HIP_TRY(m->d_colptr.upload(colptr));
            HIP_TRY(m->d_rows.upload(rows));
            HIP_TRY(m->d_pos.upload(pos));
            return MI_OK;
        }();
        if (rc != MI_OK) {
            mi_prep_destroy(m);
            return rc;
        }
        *out = m;
        return MI_OK;
    });
}

int mi_prep_info(const mi_prep_matrix *m, int *n, int *g, int64_t *nnz, int *sparse, int64_t *device_bytes)
{
    if (!m) return fail(MI_EINVAL, "NULL argument");
    if (n) *n = m->n;
    if (g) *g = m->g;
    if (nnz) *nnz = m->sparse ? m->nnz : (int64_t)m->n * m->g;
    if (sparse) *sparse = m->sparse;
    if (device_bytes)
        *device_bytes = (int64_t)((m->d_X.count + m->d_Y.count + m->d_Z.count) * sizeof(float) +
                                  (m->d_indptr.count + m->d_colptr.count) * sizeof(int64_t) +
                                  (m->d_indices.count + m->d_rows.count + m->d_pos.count) * sizeof(int32_t));
    return MI_OK;
}

int mi_prep_normalize(mi_prep_matrix *m, double scale_factor, float *out_kernel_ms)
{
    return on_matrix(m, true, 0, out_kernel_ms, [&]() -> int {
        if (!(scale_factor > 0.0) || std::isinf(scale_factor)) return fail(MI_EINVAL, "scale_factor must be finite and > 0");
        HIP_TRY(m->d_Y.reserve(m->sparse ? (size_t)m->nnz : (size_t)m->n * m->g));
        m->normalized = false;
        Timer t;
        MI_TRY(t.start(0));
        if (m->sparse)
            hipLaunchKernelGGL(k_prep_csr_normalize, dim3((unsigned)((m->n + 3) / 4)), dim3(256), 0, 0, m->d_indptr, m->d_indices,
                               m->d_X, m->d_Y, m->n, scale_factor);
        else
            hipLaunchKernelGGL(k_prep_normalize, dim3((unsigned)((m->n + 3) / 4)), dim3(256), 0, 0, m->d_X, m->d_Y, m->n, m->g,
                               scale_factor);
        MI_TRY(t.stop(0, out_kernel_ms));
        m->normalized = true;
        return MI_OK;
    });
}

int mi_prep_fetch_normalized(mi_prep_matrix *m, float *out)
{
    return on_matrix(m, out != nullptr, 0, nullptr, [&]() -> int {
        if (m->sparse) return fail(MI_EUNSUPPORTED, "a sparse handle has no dense normalised matrix: mi_prep_fetch_normalized_csr");
        MI_TRY(check_state(m, NEED_NORMALIZED));
        HIP_TRY(hipMemcpy(out, m->d_Y, (size_t)m->n * m->g * sizeof(float), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_prep_fetch_normalized_csr(mi_prep_matrix *m, float *out_data)
{
    return on_matrix(m, out_data != nullptr, 0, nullptr, [&]() -> int {
        if (!m->sparse) return fail(MI_EINVAL, "the handle is dense: mi_prep_fetch_normalized");
        MI_TRY(check_state(m, NEED_NORMALIZED));
        if (m->nnz) HIP_TRY(hipMemcpy(out_data, m->d_Y, (size_t)m->nnz * sizeof(float), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_prep_gene_stats(mi_prep_matrix *m, int which, double *mean, double *var, int32_t *nnz, float *out_kernel_ms)
{
    return on_matrix(m, true, 0, out_kernel_ms, [&]() -> int {
        if (which != 0 && which != 1) return fail(MI_EINVAL, "which must be 0 (counts) or 1 (normalised), got %d", which);
        MI_TRY(check_state(m, which ? NEED_NORMALIZED : 0));
        const size_t g = (size_t)m->g, ns = (size_t)slices(m);
        DevBufs bufs;
        double *d_psum, *d_mean, *d_var;
        int32_t *d_pnnz, *d_nnz;
        HIP_TRY(bufs.alloc(&d_psum, ns * g));
        HIP_TRY(bufs.alloc(&d_pnnz, ns * g));
        HIP_TRY(bufs.alloc(&d_mean, g));
        HIP_TRY(bufs.alloc(&d_var, g));
        HIP_TRY(bufs.alloc(&d_nnz, g));
        const float *M = which ? m->d_Y : m->d_X;
        Timer t;
        MI_TRY(t.start(0));
        MI_TRY(col_reduce(m, M, ColSum{m->g}, (double)m->n, d_psum, d_pnnz, d_mean, d_nnz));
        MI_TRY(col_reduce(m, M, ColCentred{m->g, d_mean}, (double)(m->n - 1), d_psum, nullptr, d_var, nullptr));
        MI_TRY(t.stop(0, out_kernel_ms));
        if (mean) HIP_TRY(hipMemcpy(mean, d_mean, g * sizeof(double), hipMemcpyDeviceToHost));
        if (var) HIP_TRY(hipMemcpy(var, d_var, g * sizeof(double), hipMemcpyDeviceToHost));
        if (nnz) HIP_TRY(hipMemcpy(nnz, d_nnz, g * sizeof(int32_t), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_prep_clipped_variance(mi_prep_matrix *m, const double *mean, const double *sd, double clip, double *out,
                             float *out_kernel_ms)
{
    return on_matrix(m, mean && sd && out, 0, out_kernel_ms, [&]() -> int {
        if (std::isnan(clip)) return fail(MI_EINVAL, "clip is NaN");
        for (int j = 0; j < m->g; ++j) {
            if (!std::isfinite(mean[j])) return fail(MI_EINVAL, "mean[%d] is not finite", j);
            if (!(sd[j] >= 0.0) || std::isinf(sd[j])) return fail(MI_EINVAL, "sd[%d] must be finite and >= 0", j);
        }
        const size_t g = (size_t)m->g;
        DevBufs bufs;
        double *d_psum, *d_mean, *d_sd, *d_out;
        HIP_TRY(bufs.alloc(&d_psum, (size_t)slices(m) * g));
        HIP_TRY(bufs.upload(&d_mean, mean, g));
        HIP_TRY(bufs.upload(&d_sd, sd, g));
        HIP_TRY(bufs.alloc(&d_out, g));
        Timer t;
        MI_TRY(t.start(0));
        MI_TRY(col_reduce(m, m->d_X, ColClipped{m->g, d_mean, d_sd, clip}, (double)(m->n - 1), d_psum, nullptr, d_out, nullptr));
        MI_TRY(t.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy(out, d_out, g * sizeof(double), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_prep_select(mi_prep_matrix *m, const int32_t *genes, int h, const double *mu, const double *sigma, double clip,
                   float *out_kernel_ms)
{
    return on_matrix(m, genes && mu && sigma, 0, out_kernel_ms, [&]() -> int {
        if (h < 1) return fail(MI_EINVAL, "h must be >= 1 (got %d)", h);
        if (h > MI_PREP_MAX_FEATURES) return fail(MI_EUNSUPPORTED, "%d features exceed %d", h, MI_PREP_MAX_FEATURES);
        if (!(clip > 0.0)) return fail(MI_EINVAL, "clip must be > 0");
        MI_TRY(check_indices(genes, h, m->g, "genes", "gene"));
        std::vector<uint8_t> flat((size_t)h, 0);
        std::vector<float> muf((size_t)h), inv((size_t)h);
        for (int c = 0; c < h; ++c) {
            if (!std::isfinite(mu[c])) return fail(MI_EINVAL, "mu[%d] is not finite", c);
            if (!(sigma[c] >= 0.0) || std::isinf(sigma[c])) return fail(MI_EINVAL, "sigma[%d] must be finite and >= 0", c);
            flat[c] = sigma[c] == 0.0;
            muf[c] = (float)mu[c];
            inv[c] = flat[c] ? 0.0f : (float)(1.0 / sigma[c]);
        }
        MI_TRY(check_state(m, NEED_NORMALIZED));
        m->h = 0;
        MI_TRY(size_Z(m, h));                            // (a failure leaves it empty, with h = 0: mi_prep_select has not run)
        DevBufs bufs;
        int32_t *d_genes, *d_gmap;
        float *d_mu, *d_inv;
        uint8_t *d_flat;
        MI_TRY(upload_genes(bufs, m, genes, h, &d_genes, &d_gmap));
        HIP_TRY(bufs.upload(&d_mu, muf.data(), muf.size()));
        HIP_TRY(bufs.upload(&d_inv, inv.data(), inv.size()));
        HIP_TRY(bufs.upload(&d_flat, flat.data(), flat.size()));
        Timer t;
        MI_TRY(t.start(0));
        MI_TRY(launch_select(m, m->d_Y, d_genes, d_gmap, ScaledCols{h, d_mu, d_inv, d_flat, (float)clip}));
        MI_TRY(t.stop(0, out_kernel_ms));
        m->h = h;
        return MI_OK;
    });
}

int mi_prep_cell_qc(mi_prep_matrix *m, const uint8_t *gene_mask, double *n_count, int32_t *n_feature, double *subset_count,
                    float *out_kernel_ms)
{
    return on_matrix(m, true, 0, out_kernel_ms, [&]() -> int {
        if (subset_count && !gene_mask) return fail(MI_EINVAL, "subset_count needs a gene_mask");
        for (int j = 0; gene_mask && j < m->g; ++j)
            if (gene_mask[j] > 1) return fail(MI_EINVAL, "gene_mask[%d] = %d is neither 0 nor 1", j, (int)gene_mask[j]);
        const size_t n = (size_t)m->n;
        DevBufs bufs;
        uint8_t *d_mask = nullptr;
        double *d_count, *d_subset;
        int32_t *d_feature;
        if (gene_mask) HIP_TRY(bufs.upload(&d_mask, gene_mask, (size_t)m->g));
        HIP_TRY(bufs.alloc(&d_count, n));
        HIP_TRY(bufs.alloc(&d_subset, n));
        HIP_TRY(bufs.alloc(&d_feature, n));
        Timer t;
        MI_TRY(t.start(0));
        if (m->sparse)
            hipLaunchKernelGGL(k_prep_csr_cell_qc, dim3((unsigned)((m->n + 3) / 4)), dim3(256), 0, 0, m->d_indptr, m->d_indices,
                               m->d_X, d_mask, m->n, d_count, d_feature, d_subset);
        else
            hipLaunchKernelGGL(k_prep_cell_qc, dim3((unsigned)((m->n + 3) / 4)), dim3(256), 0, 0, m->d_X, d_mask, m->n, m->g,
                               d_count, d_feature, d_subset);
        MI_TRY(t.stop(0, out_kernel_ms));
        if (n_count) HIP_TRY(hipMemcpy(n_count, d_count, n * sizeof(double), hipMemcpyDeviceToHost));
        if (n_feature) HIP_TRY(hipMemcpy(n_feature, d_feature, n * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (subset_count) HIP_TRY(hipMemcpy(subset_count, d_subset, n * sizeof(double), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_prep_select_regressed(mi_prep_matrix *m, const int32_t *genes, int h, const double *Q, int q, double clip,
                             double *out_coef, double *out_mean, double *out_var, uint8_t *out_flat, float *out_kernel_ms)
{
    return on_matrix(m, true, 0, out_kernel_ms, [&]() -> int {
        m->h = 0;                                                 // (whatever fails below, nothing is selected)
        if (!genes || !Q) return fail(MI_EINVAL, "NULL argument");
        if (h < 1) return fail(MI_EINVAL, "h must be >= 1 (got %d)", h);
        if (q < 1) return fail(MI_EINVAL, "q must be >= 1 (got %d)", q);
        if (h > MI_PREP_MAX_FEATURES) return fail(MI_EUNSUPPORTED, "%d features exceed %d", h, MI_PREP_MAX_FEATURES);
        if (q > MI_PREP_MAX_DESIGN_COLS) return fail(MI_EUNSUPPORTED, "%d design columns exceed %d", q, MI_PREP_MAX_DESIGN_COLS);
        if (!(clip > 0.0)) return fail(MI_EINVAL, "clip must be > 0");
        const size_t n = (size_t)m->n, hs = (size_t)h, qs = (size_t)q;
        MI_TRY(check_indices(genes, h, m->g, "genes", "gene"));
        MI_TRY(check_Q(Q, n, qs));
        MI_TRY(check_state(m, NEED_NORMALIZED));
        const std::vector<float> zero(hs, 0.0f), one(hs, 1.0f);
        const std::vector<uint8_t> none(hs, 0);
        MI_TRY(size_Z(m, h));                            // (a failure leaves it empty, with h = 0)
        DevBufs bufs;
        int32_t *d_genes, *d_gmap;
        float *d_mu, *d_one;
        uint8_t *d_none;
        double *d_Q;
        MI_TRY(upload_genes(bufs, m, genes, h, &d_genes, &d_gmap));
        HIP_TRY(bufs.upload(&d_mu, zero.data(), hs));
        HIP_TRY(bufs.upload(&d_one, one.data(), hs));
        HIP_TRY(bufs.upload(&d_none, none.data(), hs));
        HIP_TRY(bufs.upload(&d_Q, Q, n * qs));
        float ms1 = 0.0f, ms2 = 0.0f;
        {
            Timer t;
            MI_TRY(t.start(0));
            // 1. the gather: fminf((y - 0) * 1, inf) is y
            MI_TRY(launch_select(m, m->d_Y, d_genes, d_gmap, ScaledCols{h, d_mu, d_one, d_none, HUGE_VALF}));
            MI_TRY(t.stop(0, &ms1));
        }
        MI_TRY(regress_stages(m, h, d_Q, q, clip, false, out_coef, out_mean, out_var, out_flat, &ms2));
        if (out_kernel_ms) *out_kernel_ms = ms1 + ms2;
        m->h = h;
        return MI_OK;
    });
}

int mi_prep_fetch_scaled(mi_prep_matrix *m, float *out)
{
    return on_matrix(m, out != nullptr, NEED_SELECTED, nullptr, [&]() -> int {
        HIP_TRY(hipMemcpy2D(out, (size_t)m->h * sizeof(float), m->d_Z, (size_t)m->ldz * sizeof(float), (size_t)m->h * sizeof(float),
                            (size_t)m->n, hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_prep_gram(mi_prep_matrix *m, double *out_G, float *out_kernel_ms)
{
    return on_matrix(m, out_G != nullptr, NEED_SELECTED, out_kernel_ms, [&]() -> int {
        const int T = m->ldz / kTile, tiles = T * (T + 1) / 2;
        const int chunks = (m->n + kChunk - 1) / kChunk;
        const size_t tile_bytes = (size_t)kTile * kTile * sizeof(float), ldg = (size_t)T * kTile;
        int batch = (int)(kGramWorkspace / (tile_bytes * tiles));
        batch = batch < 1 ? 1 : (batch > chunks ? chunks : batch);
        DevBufs bufs;
        float *d_P;
        double *d_G;
        HIP_TRY(bufs.alloc(&d_P, (size_t)batch * tiles * kTile * kTile));
        HIP_TRY(bufs.alloc(&d_G, ldg * ldg));
        Timer t;
        MI_TRY(t.start(0));
        HIP_TRY(hipMemsetAsync(d_G, 0, ldg * ldg * sizeof(double), 0));
        for (int c0 = 0; c0 < chunks; c0 += batch) {
            const int nb = chunks - c0 < batch ? chunks - c0 : batch;
            hipLaunchKernelGGL(k_prep_gram, dim3((unsigned)tiles, (unsigned)nb), dim3(256), 0, 0, m->d_Z, m->ldz, m->n, T, c0, d_P);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_prep_gram_reduce, dim3((unsigned)tiles), dim3(256), 0, 0, d_P, tiles, nb, T, d_G);
            HIP_TRY(hipGetLastError());
        }
        MI_TRY(t.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy2D(out_G, (size_t)m->h * sizeof(double), d_G, ldg * sizeof(double), (size_t)m->h * sizeof(double),
                            (size_t)m->h, hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_prep_project(mi_prep_matrix *m, const float *V, int p, float *out, float *out_kernel_ms)
{
    return on_matrix(m, V && out, 0, out_kernel_ms, [&]() -> int {
        if (p < 1) return fail(MI_EINVAL, "p must be >= 1 (got %d)", p);
        if (p > MI_PREP_MAX_PCS) return fail(MI_EUNSUPPORTED, "%d output columns exceed %d", p, MI_PREP_MAX_PCS);
        MI_TRY(check_state(m, NEED_SELECTED));
        std::vector<float> Vp((size_t)m->ldz * kProjCols, 0.0f);
        for (int k = 0; k < m->h; ++k)
            for (int c = 0; c < p; ++c) {
                const float v = V[(size_t)k * p + c];
                if (!std::isfinite(v)) return fail(MI_EINVAL, "V[%d, %d] is not finite", k, c);
                Vp[(size_t)k * kProjCols + c] = v;
            }
        DevBufs bufs;
        float *d_V, *d_out;
        HIP_TRY(bufs.upload(&d_V, Vp.data(), Vp.size()));
        HIP_TRY(bufs.alloc(&d_out, (size_t)m->n * p));
        Timer t;
        MI_TRY(t.start(0));
        hipLaunchKernelGGL(k_prep_project, dim3((unsigned)((m->n + kProjCells - 1) / kProjCells)), dim3(256), 0, 0, m->d_Z, m->ldz,
                           m->n, (m->h + kKC - 1) / kKC * kKC, d_V, p, d_out);
        MI_TRY(t.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy(out, d_out, (size_t)m->n * p * sizeof(float), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_prep_gene_log1p_sum(mi_prep_matrix *m, double *out, float *out_kernel_ms)
{
    return on_matrix(m, out != nullptr, 0, out_kernel_ms, [&]() -> int {
        const size_t g = (size_t)m->g;
        DevBufs bufs;
        double *d_psum, *d_out;
        HIP_TRY(bufs.alloc(&d_psum, (size_t)slices(m) * g));
        HIP_TRY(bufs.alloc(&d_out, g));
        Timer t;
        MI_TRY(t.start(0));
        MI_TRY(col_reduce(m, m->d_X, ColLog1p{m->g}, 1.0, d_psum, nullptr, d_out, nullptr));
        MI_TRY(t.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy(out, d_out, g * sizeof(double), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_prep_nb_fit(mi_prep_matrix *m, const int32_t *cells, int mc, const int32_t *genes, int g1, const double *log_umi,
                   double *out_b0, double *out_b1, double *out_alpha, double *out_se_b0c, double *out_se_b1,
                   double *out_se_alpha, int32_t *out_iterations, uint8_t *out_converged, uint8_t *out_poisson,
                   float *out_kernel_ms)
{
    const bool args_ok = cells && genes && log_umi && out_b0 && out_b1 && out_alpha && out_se_b0c && out_se_b1 && out_se_alpha &&
                         out_iterations && out_converged && out_poisson;
    return on_matrix(m, args_ok, 0, out_kernel_ms, [&]() -> int {
        if (mc < 3) return fail(MI_EINVAL, "at least 3 fit cells are needed (got %d)", mc);
        if (g1 < 1) return fail(MI_EINVAL, "at least 1 fit gene is needed (got %d)", g1);
        if (mc > MI_PREP_SCT_MAX_FIT_CELLS) return fail(MI_EUNSUPPORTED, "%d fit cells exceed %d", mc, MI_PREP_SCT_MAX_FIT_CELLS);
        if (g1 > MI_PREP_MAX_FEATURES) return fail(MI_EUNSUPPORTED, "%d fit genes exceed %d", g1, MI_PREP_MAX_FEATURES);
        MI_TRY(check_indices(cells, mc, m->n, "cells", "cells"));
        MI_TRY(check_indices(genes, g1, m->g, "genes", "genes"));
        MI_TRY(check_log_umi(log_umi, mc));
        const size_t ms = (size_t)mc, gs = (size_t)g1;
        // the centred covariate, in host fp64: the mean is the sum in the order of `cells`, divided by their number
        double total = 0.0;
        for (int i = 0; i < mc; ++i) total += log_umi[i];
        const double xmean = total / (double)mc;
        std::vector<double> xc(ms);
        bool constant = true;
        for (int i = 0; i < mc; ++i) {
            xc[i] = log_umi[i] - xmean;
            constant = constant && log_umi[i] == log_umi[0];
        }
        if (constant) return fail(MI_EINVAL, "log_umi is the same in every fit cell: the slope is not identified");
        DevBufs bufs;
        int32_t *d_cells, *d_genes, *d_gmap, *d_iter;             // (d_gmap: gene -> row of the block)
        float *d_B;
        double *d_xc, *d_out;
        uint8_t *d_flags;
        HIP_TRY(bufs.upload(&d_cells, cells, ms));
        MI_TRY(upload_genes(bufs, m, genes, g1, &d_genes, &d_gmap));
        HIP_TRY(bufs.alloc(&d_B, ms * gs));
        HIP_TRY(bufs.upload(&d_xc, xc.data(), ms));
        HIP_TRY(bufs.alloc(&d_out, 6 * gs));
        HIP_TRY(bufs.alloc(&d_iter, gs));
        HIP_TRY(bufs.alloc(&d_flags, 2 * gs));
        Timer t;
        MI_TRY(t.start(0));
        if (m->sparse)
            hipLaunchKernelGGL(k_sct_csr_gather, dim3((unsigned)mc), dim3(256), 0, 0, m->d_indptr, m->d_indices, m->d_X, d_gmap,
                               d_cells, mc, g1, d_B);
        else
            hipLaunchKernelGGL(k_sct_gather, dim3((unsigned)((g1 + 255) / 256), (unsigned)mc), dim3(256), 0, 0, m->d_X, m->g,
                               d_cells, mc, d_genes, g1, d_B);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_sct_nb_fit, dim3((unsigned)g1), dim3(256), 0, 0, d_B, mc, d_xc, xmean, d_out, d_out + gs,
                           d_out + 2 * gs, d_out + 3 * gs, d_out + 4 * gs, d_out + 5 * gs, d_iter, d_flags, d_flags + gs);
        MI_TRY(t.stop(0, out_kernel_ms));
        double *outs[6] = {out_b0, out_b1, out_alpha, out_se_b0c, out_se_b1, out_se_alpha};
        for (int k = 0; k < 6; ++k) HIP_TRY(hipMemcpy(outs[k], d_out + k * gs, gs * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out_iterations, d_iter, gs * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out_converged, d_flags, gs, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out_poisson, d_flags + gs, gs, hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_prep_sct_residual_moments(mi_prep_matrix *m, const int32_t *genes, int gp, const double *b0, const double *b1,
                                 const double *alpha, const double *log_umi, double clip, double *out_mean, double *out_var,
                                 float *out_kernel_ms)
{
    return on_matrix(m, genes && b0 && b1 && alpha && log_umi && out_mean && out_var, 0, out_kernel_ms, [&]() -> int {
        if (gp < 1) return fail(MI_EINVAL, "at least 1 gene is needed (got %d)", gp);
        if (gp > m->g) return fail(MI_EINVAL, "%d genes are chosen of %d", gp, m->g);
        if (!(clip > 0.0)) return fail(MI_EINVAL, "clip must be > 0");
        std::vector<double> par;
        MI_TRY(check_indices(genes, gp, m->g, "genes", "genes"));
        MI_TRY(pack_nb_parameters(b0, b1, alpha, gp, par));
        MI_TRY(check_log_umi(log_umi, m->n));
        const size_t gs = (size_t)gp;
        DevBufs bufs;
        int32_t *d_genes;
        double *d_par, *d_lu, *d_psum, *d_mean, *d_var;
        HIP_TRY(bufs.upload(&d_genes, genes, gs));
        HIP_TRY(bufs.upload(&d_par, par.data(), par.size()));
        HIP_TRY(bufs.upload(&d_lu, log_umi, (size_t)m->n));
        HIP_TRY(bufs.alloc(&d_psum, (size_t)slices(m) * gs));
        HIP_TRY(bufs.alloc(&d_mean, gs));
        HIP_TRY(bufs.alloc(&d_var, gs));
        Timer t;
        MI_TRY(t.start(0));
        MI_TRY(col_reduce(m, m->d_X, SctMoment<0>{gp, d_genes, d_par, d_lu, clip, nullptr}, (double)m->n, d_psum, nullptr, d_mean,
                          nullptr));
        MI_TRY(col_reduce(m, m->d_X, SctMoment<1>{gp, d_genes, d_par, d_lu, clip, d_mean}, (double)(m->n - 1), d_psum, nullptr,
                          d_var, nullptr));
        MI_TRY(t.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy(out_mean, d_mean, gs * sizeof(double), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out_var, d_var, gs * sizeof(double), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_prep_sct_select(mi_prep_matrix *m, const int32_t *genes, int h, const double *b0, const double *b1, const double *alpha,
                       const double *log_umi, double clip, const double *Q, int q, double *out_coef, double *out_mean,
                       double *out_var, uint8_t *out_flat, float *out_kernel_ms)
{
    return on_matrix(m, true, 0, out_kernel_ms, [&]() -> int {
        m->h = 0;                                                 // (whatever fails below, nothing is selected)
        const bool raw = !Q && q == 0;                            // stage 1 alone: the residuals as they are
        if (!genes || !b0 || !b1 || !alpha || !log_umi || (!Q && !raw)) return fail(MI_EINVAL, "NULL argument");
        if (h < 1) return fail(MI_EINVAL, "h must be >= 1 (got %d)", h);
        if (q < 1 && !raw) return fail(MI_EINVAL, "q must be >= 1, or 0 without Q (got %d)", q);
        if (h > MI_PREP_MAX_FEATURES) return fail(MI_EUNSUPPORTED, "%d features exceed %d", h, MI_PREP_MAX_FEATURES);
        if (q > MI_PREP_MAX_DESIGN_COLS) return fail(MI_EUNSUPPORTED, "%d design columns exceed %d", q, MI_PREP_MAX_DESIGN_COLS);
        if (!(clip > 0.0)) return fail(MI_EINVAL, "clip must be > 0");
        const size_t n = (size_t)m->n, qs = (size_t)q;
        std::vector<double> par;
        MI_TRY(check_indices(genes, h, m->g, "genes", "genes"));
        MI_TRY(pack_nb_parameters(b0, b1, alpha, h, par));
        MI_TRY(check_log_umi(log_umi, m->n));
        MI_TRY(check_Q(Q, n, qs));
        MI_TRY(size_Z(m, h));                            // (a failure leaves it empty, with h = 0)
        DevBufs bufs;
        int32_t *d_genes, *d_gmap;
        double *d_par, *d_lu, *d_Q;
        MI_TRY(upload_genes(bufs, m, genes, h, &d_genes, &d_gmap));
        HIP_TRY(bufs.upload(&d_par, par.data(), par.size()));
        HIP_TRY(bufs.upload(&d_lu, log_umi, n));
        HIP_TRY(bufs.upload(&d_Q, Q, n * qs));                    // (raw: no columns, nothing is copied)
        float ms1 = 0.0f, ms2 = 0.0f;
        {
            Timer t;
            MI_TRY(t.start(0));
            // 1. Z = (float) the clipped residual
            MI_TRY(launch_select(m, m->d_X, d_genes, d_gmap, SctCols{h, d_par, d_lu, clip}));
            MI_TRY(t.stop(0, &ms1));
        }
        // 2 - 5. centring (and regression) by the projection off Q, unit scale, no further clip
        if (!raw) MI_TRY(regress_stages(m, h, d_Q, q, HUGE_VAL, true, out_coef, out_mean, out_var, out_flat, &ms2));
        if (out_kernel_ms) *out_kernel_ms = ms1 + ms2;
        m->h = h;
        return MI_OK;
    });
}

int mi_prep_sct_correct(mi_prep_matrix *m, const int32_t *genes, int gp, const double *b0, const double *b1,
                        const double *alpha, const double *log_umi, double log_umi_ref, mi_prep_matrix **out,
                        float *out_kernel_ms)
{
    if (out) *out = nullptr;
    return on_matrix(m, genes && b0 && b1 && alpha && log_umi && out, 0, out_kernel_ms, [&]() -> int {
        if (gp < 1) return fail(MI_EINVAL, "at least 1 gene is needed (got %d)", gp);
        if (gp > m->g) return fail(MI_EINVAL, "%d genes are chosen of %d", gp, m->g);
        std::vector<double> par;
        MI_TRY(check_indices(genes, gp, m->g, "genes", "genes"));
        MI_TRY(pack_nb_parameters(b0, b1, alpha, gp, par));
        MI_TRY(check_log_umi(log_umi, m->n));
        if (!std::isfinite(log_umi_ref)) return fail(MI_EINVAL, "log_umi_ref is not finite");
        const int n = m->n, g = m->g;
        const size_t ns = (size_t)n, gs = (size_t)g;
        DevBufs bufs;
        int32_t *d_genes, *d_count;
        double *d_par, *d_lu, *d_tab;
        uint8_t *d_listed;
        int *d_bad;
        HIP_TRY(bufs.upload(&d_genes, genes, (size_t)gp));
        HIP_TRY(bufs.upload(&d_par, par.data(), par.size()));
        HIP_TRY(bufs.upload(&d_lu, log_umi, ns));
        HIP_TRY(bufs.alloc(&d_tab, 5 * gs));
        HIP_TRY(bufs.alloc(&d_listed, gs));
        HIP_TRY(bufs.alloc(&d_bad, 1));
        HIP_TRY(bufs.alloc(&d_count, (ns > gs ? ns : gs)));       // the rows' counts, then the genes'
        HIP_TRY(hipMemset(d_tab, 0, 5 * gs * sizeof(double)));
        HIP_TRY(hipMemset(d_listed, 0, gs));
        HIP_TRY(hipMemset(d_bad, 0, sizeof(int)));
        std::unique_ptr<mi_prep_matrix> o(new mi_prep_matrix());  // (deleted on every way out but the last: the device is current)
        o->n = n; o->g = g; o->device = m->device; o->sparse = m->sparse;
        int bad = 0;
        const auto overflowed = [&]() -> int {
            HIP_TRY(hipMemcpy(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost));
            if (bad) return fail(MI_EINVAL, "a corrected count is not finite: exp(b0 + b1 log_umi) overflows or vanishes");
            return MI_OK;
        };
        const auto table = [&]() -> int {
            hipLaunchKernelGGL(k_sct_gene_table, dim3((unsigned)((gp + 255) / 256)), dim3(256), 0, 0, d_genes, d_par, gp,
                               log_umi_ref, g, d_tab, d_listed);
            HIP_TRY(hipGetLastError());
            return MI_OK;
        };
        if (!m->sparse) {
            HIP_TRY(o->d_X.resize(ns * gs));
            HIP_TRY(o->d_Y.resize(ns * gs));
            Timer t;
            MI_TRY(t.start(0));
            MI_TRY(table());
            hipLaunchKernelGGL(k_sct_correct, dim3((unsigned)((g + 63) / 64), (unsigned)slices(m)), dim3(256), 0, 0, m->d_X, n, g,
                               d_tab, d_listed, d_lu, o->d_X, o->d_Y, d_bad);
            MI_TRY(t.stop(0, out_kernel_ms));
            MI_TRY(overflowed());
        } else {
            // the row pass: count, scan into the new indptr, fill
            float ms1 = 0.0f, ms2 = 0.0f;
            int64_t total = 0, total_t = 0;
            HIP_TRY(o->d_indptr.resize(ns + 1));
            HIP_TRY(o->d_colptr.resize(gs + 1));
            {
                Timer t;
                MI_TRY(t.start(0));
                MI_TRY(table());
                hipLaunchKernelGGL(k_sct_csr_rows<0>, dim3((unsigned)n), dim3(256), 0, 0, m->d_indptr, m->d_indices, m->d_X, g, d_tab,
                                   d_listed, d_lu, d_count, nullptr, nullptr, nullptr, nullptr, d_bad);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(k_prep_scan_counts, dim3(1), dim3(1024), 0, 0, d_count, o->d_indptr, n);
                MI_TRY(t.stop(0, &ms1));
            }
            MI_TRY(overflowed());
            HIP_TRY(hipMemcpy(&total, o->d_indptr + ns, sizeof(int64_t), hipMemcpyDeviceToHost));
            if (total > MI_PREP_MAX_NNZ)
                return fail(MI_EUNSUPPORTED, "%lld corrected entries exceed %lld", (long long)total, (long long)MI_PREP_MAX_NNZ);
            const size_t nz = (size_t)total;
            HIP_TRY(o->d_indices.resize(nz));
            HIP_TRY(o->d_X.resize(nz));
            HIP_TRY(o->d_Y.resize(nz));
            HIP_TRY(o->d_rows.resize(nz));
            HIP_TRY(o->d_pos.resize(nz));
            // the transpose, by counting sort of what the row pass wrote.  Blocks of R rows: about a thousand workgroups, at
            // least 32 rows each, the histogram (blocks x genes, scratch) within 2^26 counts
            const long long nb_max = std::max(1ll, (1ll << 26) / (long long)g);
            const int R = (int)std::max({32ll, ((long long)n + 1023) / 1024, ((long long)n + nb_max - 1) / nb_max});
            const int nb = (n + R - 1) / R;
            int32_t *d_hist;
            HIP_TRY(bufs.alloc(&d_hist, (size_t)nb * gs));
            {
                Timer t;
                MI_TRY(t.start(0));
                hipLaunchKernelGGL(k_sct_csr_rows<1>, dim3((unsigned)n), dim3(256), 0, 0, m->d_indptr, m->d_indices, m->d_X, g, d_tab,
                                   d_listed, d_lu, nullptr, o->d_indptr, o->d_indices, o->d_X, o->d_Y, d_bad);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipMemsetAsync(d_hist, 0, (size_t)nb * gs * sizeof(int32_t), 0));
                hipLaunchKernelGGL(k_csr_block_hist, dim3((unsigned)nb), dim3(256), 0, 0, o->d_indptr, o->d_indices, n, g, R, d_hist);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(k_csr_block_offsets, dim3((unsigned)((g + 255) / 256)), dim3(256), 0, 0, d_hist, nb, g, d_count);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(k_prep_scan_counts, dim3(1), dim3(1024), 0, 0, d_count, o->d_colptr, g);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(k_csr_block_transpose, dim3((unsigned)nb), dim3(256), 0, 0, o->d_indptr, o->d_indices, n, g, R,
                                   o->d_colptr, d_hist, o->d_rows, o->d_pos);
                MI_TRY(t.stop(0, &ms2));
            }
            HIP_TRY(hipMemcpy(&total_t, o->d_colptr + gs, sizeof(int64_t), hipMemcpyDeviceToHost));
            if (total_t != total)
                return fail(MI_EHIP, "the transpose holds %lld entries, the rows %lld", (long long)total_t, (long long)total);
            o->nnz = total;
            if (out_kernel_ms) *out_kernel_ms = ms1 + ms2;
        }
        o->normalized = true;
        *out = o.release();
        return MI_OK;
    });
}

int mi_prep_fetch_counts(mi_prep_matrix *m, float *out)
{
    return on_matrix(m, out != nullptr, 0, nullptr, [&]() -> int {
        if (m->sparse) return fail(MI_EUNSUPPORTED, "a sparse handle has no dense matrix of counts: mi_prep_fetch_csr");
        HIP_TRY(hipMemcpy(out, m->d_X, (size_t)m->n * m->g * sizeof(float), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_prep_fetch_csr(mi_prep_matrix *m, int64_t *indptr, int32_t *indices, float *data)
{
    return on_matrix(m, true, 0, nullptr, [&]() -> int {
        if (!m->sparse) return fail(MI_EINVAL, "the handle is dense: mi_prep_fetch_counts");
        const size_t nz = (size_t)m->nnz;
        if (indptr) HIP_TRY(hipMemcpy(indptr, m->d_indptr, ((size_t)m->n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
        if (indices && nz) HIP_TRY(hipMemcpy(indices, m->d_indices, nz * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (data && nz) HIP_TRY(hipMemcpy(data, m->d_X, nz * sizeof(float), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

}  // extern "C"
