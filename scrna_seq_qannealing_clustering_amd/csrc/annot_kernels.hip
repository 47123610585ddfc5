// annot_kernels.hip -- reference-based cell-type annotation: Spearman scores on marker genes, per-label quantile, fine-tuning
// (gfx950).  C ABI: include/mi_annot.h; the specification is DESIGN.md section 5c ("chain A"); markers and pruning are host
// fp64 in annotate.py.
//
// A row (a reference sample or a test cell) is ranked over a set of genes with midranks, kept doubled (r2), by the scheme of
// mi_midrank.h (wg_midranks, the sort array in LDS): the non-zeros get their r2 from a sort, the zeros of a row (both signs)
// are one tie block with a closed-form r2.
//
//   k_annot_rank       one workgroup per row over the m marker genes: r2 as two base-128 digits (2 <= r2 <= 2 m <= 16382 <
//                      128^2) in two i8 planes of mpad = 64 ceil(m / 64) bytes per row (padding 0), and sum r2^2.
//   k_annot_cross      one wavefront per 16 cells x 64 samples: per 64 genes the four digit products hi.hi, hi.lo, lo.hi, lo.lo
//                      on v_mfma_i32_16x16x64_i8 (each sum at most 127^2 * 8191 < 2^31), combined as 16384 hh + 128 (hl + lh)
//                      + ll in int64.  Operand maps as in agreement_kernels.hip: lane l holds A[row l & 15][16 genes of lane
//                      group l >> 4] and B[the same genes][col l & 15]; register q of the accumulator is C[row 4 (l >> 4) + q]
//                      [col l & 15].  Both operands read 16 contiguous bytes of their row.  Rows past the end read the last
//                      row and are dropped.
//   k_annot_scores     one workgroup per cell: rho per sample in fp64 from the integers (num = m sab - (sum)^2, da, db in int64,
//                      rho = (double)num / sqrt((double)da * (double)db), 0 when da or db is 0), then per label the 0.8
//                      quantile of its samples' rho (the samples are grouped by label on upload; the two order statistics are
//                      found by counting, which needs no sort and does not depend on thread order), then the argmax.
//   k_annot_fine_tune  one workgroup per cell, the loop of the specification: G' = OR of the pair masks of the labels in use,
//                      the cell ranked over G' (rank_row through the gene list), then every sample of the labels in use
//                      ranked over G' by the whole workgroup, one after another; its sorted positions yield sum a b and sum
//                      b^2 directly (the zero block's share is closed-form), so no rank array of the sample is kept.  At most
//                      L iterations: `use` strictly shrinks or the loop stops.
// The chunk may come from a resident mi_prep_matrix (mi_annot_score_matrix, mi_annot_score_clusters) with no host traffic:
//   k_annot_gather_dense  chunk[i][s] = V[(row0 + i) g + cols[s]]: thread = slot, blockIdx.y = cell, 64-bit element indices.
//   k_annot_gather_csr    one workgroup per cell, as k_prep_csr_select: the row's m value words zeroed in LDS, a barrier, the
//                         cell's stored entries whose gene has a slot (gmap: g int32, -1 = absent) written over their slot
//                         (the columns of a row are distinct: no two entries share a slot), a barrier, one coalesced store.
//   k_annot_means<Src>    one wavefront per (slot, block of 64 clusters), lane = cluster.  The gene's entries (the n cells of
//                         a dense column; the stored entries of the transpose, rows ascending) are fetched 64 at a time, one
//                         per lane, then handed round in entry order: every lane adds entry j in fp64 when its cell's label
//                         is the lane's cluster.  Each (cluster, slot) sum is therefore the sequential fp64 sum in ascending
//                         cell index of the specification; a skipped zero would add +0.0 to a non-negative sum, so both
//                         sources give the same bits.  mean = (float)(sum / (double)size).
// Sums are integers (any order gives the same value) or fp64 expressions of one thread; integer LDS traffic and atomics only
// in the gather; ordinary vector stores.
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/mi_annot.h"
#include "mi_midrank.h"
#include "mi_prep_handle.h"
#include "mi_sa_device.h"

namespace mi_sa_impl {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kAnnotThreads = 256;
constexpr int kAnnotWaves = kAnnotThreads / 64;
constexpr int kCrossCols = 4;                  // 16-sample tiles per wavefront of k_annot_cross
constexpr double kTuneThresh = 0.05;
constexpr double kQuantile = 0.8;

using mi_midrank::pow2_at_least;

// Whole workgroup: mi_midrank::wg_midranks on a row whose entry k of `count` has the value bits val(k).  emit(k, r2) is
// called once for every non-zero entry, by the thread that owns its sorted position.  S: pow2_at_least(count) entries of
// LDS; cnt: 2 words of LDS.  Ends with a barrier: S and cnt are free again.
template <class Val, class Emit>
__device__ __forceinline__ mi_midrank::Ranked rank_row(int count, Val val, unsigned long long *S, uint32_t *cnt, Emit emit)
{
    const mi_midrank::Ranked rk = mi_midrank::wg_midranks(
        count, val, [](int k) { return k; }, count, pow2_at_least(count), S, cnt,
        [&](int, unsigned long long e, int, int, uint32_t r2) { emit((int)(uint32_t)e, r2); });
    __syncthreads();
    return rk;
}

// the sum of N integers per thread over the workgroup; ws: N * kAnnotWaves words of LDS.  Ends with a barrier.
template <int N>
__device__ __forceinline__ void block_sums(long long (&v)[N], long long *ws)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        for (int off = 32; off > 0; off >>= 1) v[i] += __shfl_xor(v[i], off);
        if (lane == 0) ws[i * kAnnotWaves + wave] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) {
        long long s = 0;
        for (int w = 0; w < kAnnotWaves; ++w) s += ws[i * kAnnotWaves + w];
        v[i] = s;
    }
    __syncthreads();
}

// rho of doubled midranks over m genes from their exact sums; sum a = sum b = m (m + 1)
__device__ __forceinline__ double spearman(long long m, long long sab, long long sa2, long long sb2)
{
    const long long sum = m * (m + 1);
    const long long num = m * sab - sum * sum, da = m * sa2 - sum * sum, db = m * sb2 - sum * sum;
    if (da == 0 || db == 0) return 0.0;
    return (double)num / sqrt((double)da * (double)db);
}

// sc[l] = the 0.8 quantile of rho over the samples off[l] .. off[l + 1] - 1, for every label l of `use`.  Whole workgroup;
// the order statistics c[lo] and c[min(lo + 1, s - 1)] are the entries whose place by counting (smaller values, then equal
// values of lower index) is lo, lo + 1.  Ends with a barrier.
__device__ __forceinline__ void label_quantiles(const double *rho, const int *off, int L, unsigned long long use, double *qlo,
                                                double *qhi, double *sc)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int l = 0; l < L; ++l) {
        if (!((use >> l) & 1ull)) continue;
        const int o = off[l], s = off[l + 1] - o;
        const int lo = (int)floor(kQuantile * (double)(s - 1)), hi = lo + 1 < s - 1 ? lo + 1 : s - 1;
        for (int i = tid; i < s; i += nt) {
            const double c = rho[o + i];
            int place = 0;
            for (int j = 0; j < s; ++j) {
                const double d = rho[o + j];
                place += (d < c || (d == c && j < i)) ? 1 : 0;
            }
            if (place == lo) qlo[l] = c;
            if (place == hi) qhi[l] = c;
        }
    }
    __syncthreads();
    if (tid < L && ((use >> tid) & 1ull)) {
        const int s = off[tid + 1] - off[tid];
        const double pos = kQuantile * (double)(s - 1);
        sc[tid] = qlo[tid] + (pos - floor(pos)) * (qhi[tid] - qlo[tid]);
    }
    __syncthreads();
}

struct RankArgs {
    const float *X = nullptr;              // rows x m
    int rows = 0, m = 0, mpad = 0, cap = 0;
    int8_t *hi = nullptr, *lo = nullptr;   // rows x mpad digit planes
    long long *s2 = nullptr;               // rows
};

__global__ void __launch_bounds__(kAnnotThreads) k_annot_rank(RankArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    unsigned long long *S = reinterpret_cast<unsigned long long *>(lds);
    uint16_t *r = reinterpret_cast<uint16_t *>(lds + (size_t)a.cap * 8);
    long long *ws = reinterpret_cast<long long *>(lds + (size_t)a.cap * 8 + (size_t)a.mpad * 2);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(ws + kAnnotWaves);
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int row = blockIdx.x; row < a.rows; row += gridDim.x) {
        const float *x = a.X + (size_t)row * a.m;
        for (int j = tid; j < a.mpad; j += nt) r[j] = 0;                                  // (0 is no rank: filled in below)
        const uint32_t zr2 = rank_row(a.m, [&](int k) { return __float_as_uint(x[k]); }, S, cnt,
                                      [&](int k, uint32_t r2) { r[k] = (uint16_t)r2; }).zero_r2;
        long long part[1] = {0};
        for (int j = tid * 4; j < a.mpad; j += nt * 4) {
            uint32_t wh = 0u, wl = 0u;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                uint32_t v = 0u;
                if (j + q < a.m) {
                    v = r[j + q];
                    if (!v) v = zr2;
                }
                wh |= (v >> 7) << (8 * q);
                wl |= (v & 127u) << (8 * q);
                part[0] += (long long)v * v;
            }
            *reinterpret_cast<uint32_t *>(a.hi + (size_t)row * a.mpad + j) = wh;
            *reinterpret_cast<uint32_t *>(a.lo + (size_t)row * a.mpad + j) = wl;
        }
        block_sums<1>(part, ws);
        if (tid == 0) a.s2[row] = part[0];
    }
}

struct CrossArgs {
    const int8_t *ahi = nullptr, *alo = nullptr, *bhi = nullptr, *blo = nullptr;
    int n = 0, S = 0, mpad = 0;
    long long *sab = nullptr;              // n x S
};

__global__ void __launch_bounds__(kAnnotThreads) k_annot_cross(CrossArgs a)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, grp = lane >> 4, l16 = lane & 15;
    const int tn = (a.n + 15) / 16, ts = (a.S + 16 * kCrossCols - 1) / (16 * kCrossCols);
    const long long tiles = (long long)tn * ts;
    for (long long t = (long long)blockIdx.x * kAnnotWaves + wave; t < tiles; t += (long long)gridDim.x * kAnnotWaves) {
        const int ti = (int)(t / ts), tj = (int)(t - (long long)ti * ts);
        const int row = ti * 16 + l16 < a.n ? ti * 16 + l16 : a.n - 1;
        const size_t oa = (size_t)row * a.mpad + 16 * grp;
        size_t ob[kCrossCols];
#pragma unroll
        for (int c = 0; c < kCrossCols; ++c) {
            const int col = (tj * kCrossCols + c) * 16 + l16;
            ob[c] = (size_t)(col < a.S ? col : a.S - 1) * a.mpad + 16 * grp;
        }
        i32x4 hh[kCrossCols], hl[kCrossCols], lh[kCrossCols], ll[kCrossCols];
#pragma unroll
        for (int c = 0; c < kCrossCols; ++c) hh[c] = hl[c] = lh[c] = ll[c] = i32x4{0, 0, 0, 0};
        for (int k0 = 0; k0 < a.mpad; k0 += 64) {
            const i32x4 ah = *reinterpret_cast<const i32x4 *>(a.ahi + oa + k0);
            const i32x4 al = *reinterpret_cast<const i32x4 *>(a.alo + oa + k0);
#pragma unroll
            for (int c = 0; c < kCrossCols; ++c) {
                const i32x4 bh = *reinterpret_cast<const i32x4 *>(a.bhi + ob[c] + k0);
                const i32x4 bl = *reinterpret_cast<const i32x4 *>(a.blo + ob[c] + k0);
                hh[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bh, hh[c], 0, 0, 0);
                hl[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(ah, bl, hl[c], 0, 0, 0);
                lh[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bh, lh[c], 0, 0, 0);
                ll[c] = __builtin_amdgcn_mfma_i32_16x16x64_i8(al, bl, ll[c], 0, 0, 0);
            }
        }
#pragma unroll
        for (int c = 0; c < kCrossCols; ++c) {
            const int col = (tj * kCrossCols + c) * 16 + l16;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int rw = ti * 16 + 4 * grp + q;
                if (rw < a.n && col < a.S)
                    a.sab[(size_t)rw * a.S + col] = 16384ll * hh[c][q] + 128ll * ((long long)hl[c][q] + (long long)lh[c][q]) + (long long)ll[c][q];
            }
        }
    }
}

struct ScoreArgs {
    const long long *sab = nullptr, *sa2 = nullptr, *sb2 = nullptr;
    const int32_t *off = nullptr;          // L + 1: the samples of label l are off[l] .. off[l + 1] - 1
    int n = 0, S = 0, L = 0, m = 0;
    double *scores = nullptr;              // n x L
    int32_t *first = nullptr;              // n
};

__global__ void __launch_bounds__(kAnnotThreads) k_annot_scores(ScoreArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    double *rho = reinterpret_cast<double *>(lds);
    double *sc = rho + ((a.S + 1) & ~1), *qlo = sc + 64, *qhi = qlo + 64;
    const int tid = threadIdx.x, nt = blockDim.x;
    const unsigned long long all = a.L >= 64 ? ~0ull : (1ull << a.L) - 1ull;
    for (int cell = blockIdx.x; cell < a.n; cell += gridDim.x) {
        const long long sa2 = a.sa2[cell];
        for (int s = tid; s < a.S; s += nt) rho[s] = spearman(a.m, a.sab[(size_t)cell * a.S + s], sa2, a.sb2[s]);
        __syncthreads();
        label_quantiles(rho, a.off, a.L, all, qlo, qhi, sc);
        for (int l = tid; l < a.L; l += nt) a.scores[(size_t)cell * a.L + l] = sc[l];
        if (tid == 0) {
            int best = 0;
            for (int l = 1; l < a.L; ++l)
                if (sc[l] > sc[best]) best = l;
            a.first[cell] = best;
        }
        __syncthreads();
    }
}

struct TuneArgs {
    const float *X = nullptr, *R = nullptr;    // n x m cells, S x m samples grouped by label
    const int32_t *off = nullptr;
    const uint32_t *masks = nullptr;           // L * L rows of W words
    const double *scores = nullptr;            // n x L
    int n = 0, S = 0, L = 0, m = 0, W = 0, mpad = 0, cap = 0;
    int32_t *labels = nullptr, *iters = nullptr;
    double *best = nullptr, *next = nullptr;
};

__host__ __device__ inline size_t tune_lds_bytes(int cap, int mpad, int W, int S)
{
    return (size_t)cap * 8 + (size_t)mpad * 4 + (size_t)((W + 3) & ~3) * 8 + (size_t)((S + 1) & ~1) * 8 + 3 * 64 * 8 +
           3 * kAnnotWaves * 8 + 16;
}

__global__ void __launch_bounds__(kAnnotThreads) k_annot_fine_tune(TuneArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int Wp = (a.W + 3) & ~3;
    unsigned long long *Sx = reinterpret_cast<unsigned long long *>(lds);
    uint16_t *ar = reinterpret_cast<uint16_t *>(lds + (size_t)a.cap * 8);                 // the cell's r2 per gene of G'
    uint16_t *gidx = ar + a.mpad;                                                         // the genes of G', ascending
    uint32_t *gmask = reinterpret_cast<uint32_t *>(gidx + a.mpad);
    uint32_t *gpre = gmask + Wp;
    double *rho = reinterpret_cast<double *>(gpre + Wp);
    double *sc = rho + ((a.S + 1) & ~1), *qlo = sc + 64, *qhi = qlo + 64;
    long long *ws = reinterpret_cast<long long *>(qhi + 64);
    uint32_t *cnt = reinterpret_cast<uint32_t *>(ws + 3 * kAnnotWaves);                   // [0], [1]: rank_row; [2]: |G'|
    const int tid = threadIdx.x, nt = blockDim.x, L = a.L, W = a.W;
    const unsigned long long all = L >= 64 ? ~0ull : (1ull << L) - 1ull;

    // the labels of `set` whose score is within the threshold of the set's largest (every thread: uniform)
    auto within = [&](unsigned long long set) {
        double mx = -HUGE_VAL;
        for (int l = 0; l < L; ++l)
            if (((set >> l) & 1ull) && sc[l] > mx) mx = sc[l];
        const double thr = mx - kTuneThresh;
        unsigned long long out = 0ull;
        for (int l = 0; l < L; ++l)
            if (((set >> l) & 1ull) && sc[l] >= thr) out |= 1ull << l;
        return out;
    };

    for (int cell = blockIdx.x; cell < a.n; cell += gridDim.x) {
        for (int l = tid; l < L; l += nt) sc[l] = a.scores[(size_t)cell * L + l];
        __syncthreads();
        unsigned long long last = all, use = within(all);
        int iters = 0;
        const float *x = a.X + (size_t)cell * a.m;
        while (__popcll(use) > 1) {
            for (int w = tid; w < W; w += nt) {
                uint32_t u = 0u;
                for (int p = 0; p < L; ++p) {
                    if (!((use >> p) & 1ull)) continue;
                    for (int q = 0; q < L; ++q)
                        if (q != p && ((use >> q) & 1ull)) u |= a.masks[((size_t)p * L + q) * W + w];
                }
                gmask[w] = u;
            }
            __syncthreads();
            if (tid == 0) {
                uint32_t run = 0u;
                for (int w = 0; w < W; ++w) {
                    gpre[w] = run;
                    run += (uint32_t)__popc(gmask[w]);
                }
                cnt[2] = run;
            }
            __syncthreads();
            const int mp = (int)cnt[2];
            for (int w = tid; w < W; w += nt) {
                uint32_t u = gmask[w], k = gpre[w];
                while (u) {
                    gidx[k++] = (uint16_t)(w * 32 + __ffs((int)u) - 1);
                    u &= u - 1u;
                }
            }
            for (int k = tid; k < mp; k += nt) ar[k] = 0;
            __syncthreads();

            const uint32_t zr2 = rank_row(mp, [&](int k) { return __float_as_uint(x[gidx[k]]); }, Sx, cnt,
                                          [&](int k, uint32_t r2) { ar[k] = (uint16_t)r2; }).zero_r2;
            long long pa[1] = {0};
            for (int k = tid; k < mp; k += nt) {
                uint32_t v = ar[k];
                if (!v) {
                    v = zr2;
                    ar[k] = (uint16_t)v;
                }
                pa[0] += (long long)v * v;
            }
            block_sums<1>(pa, ws);                                                       // (its barriers publish ar)
            const long long sa2 = pa[0], sum = (long long)mp * (mp + 1);

            for (int l = 0; l < L; ++l) {
                if (!((use >> l) & 1ull)) continue;
                for (int s = a.off[l]; s < a.off[l + 1]; ++s) {
                    const float *rr = a.R + (size_t)s * a.m;
                    long long pv[3] = {0, 0, 0};                                         // sum a b, sum b^2, sum a over the sample's non-zeros
                    const mi_midrank::Ranked rk = rank_row(mp, [&](int k) { return __float_as_uint(rr[gidx[k]]); }, Sx, cnt,
                                                           [&](int k, uint32_t r2) {
                                                               const long long av = ar[k];
                                                               pv[0] += av * (long long)r2;
                                                               pv[1] += (long long)r2 * r2;
                                                               pv[2] += av;
                                                           });
                    block_sums<3>(pv, ws);
                    if (tid == 0) {
                        const long long sab = pv[0] + (sum - pv[2]) * (long long)rk.zero_r2;
                        const long long sb2 = pv[1] + (long long)rk.zeros * rk.zero_r2 * rk.zero_r2;
                        rho[s] = spearman(mp, sab, sa2, sb2);
                    }
                }
            }
            __syncthreads();
            label_quantiles(rho, a.off, L, use, qlo, qhi, sc);
            ++iters;
            last = use;
            const unsigned long long nw = within(use);
            if (nw == use) break;
            use = nw;
        }
        if (tid == 0) {
            int best = -1;
            for (int l = 0; l < L; ++l)
                if (((last >> l) & 1ull) && (best < 0 || sc[l] > sc[best])) best = l;
            double nx = -HUGE_VAL;
            for (int l = 0; l < L; ++l)
                if (((last >> l) & 1ull) && l != best && sc[l] > nx) nx = sc[l];
            a.labels[cell] = best;
            a.best[cell] = sc[best];
            a.next[cell] = nx;
            a.iters[cell] = iters;
        }
        __syncthreads();
    }
}

// ---- the chunk from a resident expression handle ---------------------------------------------------------------------------

__global__ void __launch_bounds__(kAnnotThreads) k_annot_gather_dense(const float *__restrict__ V, long long g, int row0,
                                                                      const int32_t *__restrict__ cols, int n_c, int m,
                                                                      float *__restrict__ X)
{
    const int s = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    for (int i = blockIdx.y; i < n_c; i += gridDim.y)
        if (s < m) X[(size_t)i * m + s] = V[(size_t)((long long)(row0 + i) * g + cols[s])];
}

__global__ void __launch_bounds__(kAnnotThreads) k_annot_gather_csr(const int64_t *__restrict__ indptr,
                                                                    const int32_t *__restrict__ indices,
                                                                    const float *__restrict__ vals,
                                                                    const int32_t *__restrict__ gmap, int row0, int n_c, int m,
                                                                    float *__restrict__ X)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    uint32_t *row = reinterpret_cast<uint32_t *>(lds);                                     // m value words
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int i = blockIdx.x; i < n_c; i += gridDim.x) {
        for (int s = tid; s < m; s += nt) row[s] = 0u;
        __syncthreads();
        const int64_t e1 = indptr[(size_t)row0 + i + 1];
        for (int64_t e = indptr[(size_t)row0 + i] + tid; e < e1; e += nt) {
            const int s = gmap[indices[e]];
            if (s >= 0) row[s] = __float_as_uint(vals[e]);
        }
        __syncthreads();
        for (int s = tid; s < m; s += nt) X[(size_t)i * m + s] = __uint_as_float(row[s]);
        __syncthreads();
    }
}

// the entries of one gene in ascending cell order: entry k of count(col) is the value at(col, k).v of cell at(col, k).cell
struct ColEntry {
    float v;
    int cell;
};

struct DenseColumn {
    const float *V = nullptr;
    int n = 0;
    long long g = 0;
    __device__ int count(int) const { return n; }
    __device__ ColEntry at(int col, int k) const { return ColEntry{V[(size_t)((long long)k * g + col)], k}; }
};

struct CscColumn {
    const int64_t *colptr = nullptr;
    const int32_t *rows = nullptr, *pos = nullptr;
    const float *V = nullptr;                                                              // in the CSR order: entry pos[e]
    __device__ int count(int col) const { return (int)(colptr[col + 1] - colptr[col]); }
    __device__ ColEntry at(int col, int k) const
    {
        const int64_t e = colptr[col] + k;
        return ColEntry{V[pos[e]], rows[e]};
    }
};

template <class Src>
__global__ void __launch_bounds__(kAnnotThreads) k_annot_means(Src src, const int32_t *__restrict__ cols,
                                                               const int32_t *__restrict__ cluster_of,
                                                               const int32_t *__restrict__ sizes, int K, int m,
                                                               float *__restrict__ X)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int s = (int)blockIdx.x * kAnnotWaves + wave, c = (int)blockIdx.y * 64 + lane;   // (no barrier below: a wavefront may leave)
    if (s >= m) return;
    const int col = cols[s], count = src.count(col);
    double sum = 0.0;
    for (int k0 = 0; k0 < count; k0 += 64) {
        float v = 0.0f;
        int lab = -1;
        if (k0 + lane < count) {
            const ColEntry e = src.at(col, k0 + lane);
            v = e.v;
            lab = cluster_of[e.cell];
        }
        const int left = count - k0 < 64 ? count - k0 : 64;
        for (int j = 0; j < left; ++j) {
            const float vj = __shfl(v, j);
            const int lj = __shfl(lab, j);
            if (lj == c) sum += (double)vj;
        }
    }
    if (c < K) X[(size_t)c * m + s] = (float)(sum / (double)sizes[c]);
}

// entries of the LDS sort array for rows of m genes (at least 2: the arrays carved after it stay 16-byte aligned)
inline int sort_cap(int m) { return m > 2 ? pow2_at_least(m) : 2; }

// ranks `rows` rows of d_X (rows x m) into the digit planes and s2
int launch_rank(const float *d_X, int rows, int m, int mpad, int8_t *hi, int8_t *lo, long long *s2)
{
    RankArgs a;
    a.X = d_X; a.rows = rows; a.m = m; a.mpad = mpad; a.cap = sort_cap(m); a.hi = hi; a.lo = lo; a.s2 = s2;
    const size_t bytes = (size_t)a.cap * 8 + (size_t)mpad * 2 + kAnnotWaves * 8 + 16;
    MI_TRY(allow_lds(k_annot_rank, bytes));
    hipLaunchKernelGGL(k_annot_rank, dim3((unsigned)rows), dim3(kAnnotThreads), bytes, 0, a);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

bool finite_bits(const float *v, size_t count, size_t *bad)
{
    const uint32_t *u = reinterpret_cast<const uint32_t *>(v);
    for (size_t e = 0; e < count; ++e)
        if ((u[e] & 0x7f800000u) == 0x7f800000u) {
            *bad = e;
            return false;
        }
    return true;
}

}  // namespace
}  // namespace mi_sa_impl
using namespace mi_sa_impl;

struct mi_annot {
    int S = 0, m = 0, L = 0, W = 0, mpad = 0, device = 0, cus = 0;
    int n_c = 0;                               // cells of the resident chunk (0: none yet)
    std::vector<int32_t> perm;                 // grouped position -> the caller's sample index
    DevArray<float> d_R, d_X;                  // S x m grouped by label; the chunk
    DevArray<int8_t> d_rhi, d_rlo, d_chi, d_clo;
    DevArray<long long> d_sb2, d_sa2, d_sab;
    DevArray<int32_t> d_off, d_first, d_labels, d_iters;
    DevArray<uint32_t> d_masks;
    DevArray<double> d_scores, d_best, d_next;
};

namespace {

// the chunk and everything the chain writes per cell, for n_c cells (contents are not kept)
int reserve_chunk(mi_annot *h, int n_c)
{
    HIP_TRY(h->d_X.reserve((size_t)n_c * h->m));
    HIP_TRY(h->d_chi.reserve((size_t)n_c * h->mpad));
    HIP_TRY(h->d_clo.reserve((size_t)n_c * h->mpad));
    HIP_TRY(h->d_sa2.reserve((size_t)n_c));
    HIP_TRY(h->d_sab.reserve((size_t)n_c * h->S));
    HIP_TRY(h->d_scores.reserve((size_t)n_c * h->L));
    HIP_TRY(h->d_first.reserve((size_t)n_c));
    return MI_OK;
}

// The chain on the n_c rows of h->d_X (after reserve_chunk): ranking, cross and score kernels, whose times go to
// out_kernel_ms[0 .. 2] (nullable); the chunk is resident once they have run; then the downloads the caller asked for.
int score_chunk(mi_annot *h, int n_c, int64_t *out_sab, int64_t *out_sa2, int64_t *out_sb2, double *out_scores,
                int32_t *out_first, float *out_kernel_ms)
{
    const int S = h->S, m = h->m, L = h->L, mpad = h->mpad;
    {
        Timer tm;
        MI_TRY(tm.start(0));
        MI_TRY(launch_rank(h->d_X, n_c, m, mpad, h->d_chi, h->d_clo, h->d_sa2));
        MI_TRY(tm.stop(0, out_kernel_ms ? out_kernel_ms + 0 : nullptr));
    }
    {
        CrossArgs a;
        a.ahi = h->d_chi; a.alo = h->d_clo; a.bhi = h->d_rhi; a.blo = h->d_rlo;
        a.n = n_c; a.S = S; a.mpad = mpad; a.sab = h->d_sab;
        const long long tiles = (long long)((n_c + 15) / 16) * ((S + 16 * kCrossCols - 1) / (16 * kCrossCols));
        const long long need = (tiles + kAnnotWaves - 1) / kAnnotWaves, most = (long long)(h->cus > 0 ? h->cus : 256) * 8;
        Timer tm;
        MI_TRY(tm.start(0));
        hipLaunchKernelGGL(k_annot_cross, dim3((unsigned)(need < most ? need : most)), dim3(kAnnotThreads), 0, 0, a);
        MI_TRY(tm.stop(0, out_kernel_ms ? out_kernel_ms + 1 : nullptr));
    }
    {
        ScoreArgs a;
        a.sab = h->d_sab; a.sa2 = h->d_sa2; a.sb2 = h->d_sb2; a.off = h->d_off;
        a.n = n_c; a.S = S; a.L = L; a.m = m; a.scores = h->d_scores; a.first = h->d_first;
        const size_t bytes = (size_t)((S + 1) & ~1) * 8 + 3 * 64 * 8;
        Timer tm;
        MI_TRY(tm.start(0));
        hipLaunchKernelGGL(k_annot_scores, dim3((unsigned)n_c), dim3(kAnnotThreads), bytes, 0, a);
        MI_TRY(tm.stop(0, out_kernel_ms ? out_kernel_ms + 2 : nullptr));
    }
    h->n_c = n_c;
    if (out_sab) {
        std::vector<long long> g((size_t)n_c * S);
        HIP_TRY(hipMemcpy(g.data(), h->d_sab, g.size() * sizeof(long long), hipMemcpyDeviceToHost));
        for (int i = 0; i < n_c; ++i)
            for (int p = 0; p < S; ++p) out_sab[(size_t)i * S + h->perm[p]] = g[(size_t)i * S + p];
    }
    if (out_sa2) HIP_TRY(hipMemcpy(out_sa2, h->d_sa2, (size_t)n_c * sizeof(long long), hipMemcpyDeviceToHost));
    if (out_sb2) {
        std::vector<long long> g((size_t)S);
        HIP_TRY(hipMemcpy(g.data(), h->d_sb2, g.size() * sizeof(long long), hipMemcpyDeviceToHost));
        for (int p = 0; p < S; ++p) out_sb2[h->perm[p]] = g[p];
    }
    if (out_scores) HIP_TRY(hipMemcpy(out_scores, h->d_scores, (size_t)n_c * L * sizeof(double), hipMemcpyDeviceToHost));
    if (out_first) HIP_TRY(hipMemcpy(out_first, h->d_first, (size_t)n_c * sizeof(int32_t), hipMemcpyDeviceToHost));
    return MI_OK;
}

// The checks mi_annot_score_matrix and mi_annot_score_clusters share on (M, which), after the NULL checks: which, the device.
int check_source(const mi_annot *h, const mi_prep_matrix *M, int which)
{
    if (which != MI_PREP_MARKERS_COUNTS && which != MI_PREP_MARKERS_NORMALIZED)
        return fail(MI_EINVAL, "which must be 0 (counts) or 1 (normalised), got %d", which);
    if (M->device != h->device) return fail(MI_EINVAL, "the matrix is on device %d, the annotator on device %d", M->device, h->device);
    return MI_OK;
}

// cols: m indices in [0, g), no repeats -> gmap (g entries): the slot of every gene, -1 = absent
int check_cols(const int32_t *cols, int m, int g, std::vector<int32_t> &gmap)
{
    gmap.assign((size_t)g, -1);
    for (int s = 0; s < m; ++s) {
        if (cols[s] < 0 || cols[s] >= g) return fail(MI_EINVAL, "column %d (slot %d) is not in [0, %d)", cols[s], s, g);
        if (gmap[cols[s]] >= 0) return fail(MI_EINVAL, "column %d is repeated (slots %d and %d)", cols[s], gmap[cols[s]], s);
        gmap[cols[s]] = s;
    }
    return MI_OK;
}

}  // namespace

extern "C" {

int mi_annot_destroy(mi_annot *h)
{
    if (!h) return MI_OK;
    (void)hipSetDevice(h->device);
    delete h;
    return MI_OK;
}

int mi_annot_create(const float *R, int S, int m, const int32_t *labels, int L, const uint32_t *pair_masks, int device,
                    mi_annot **out, float *out_kernel_ms)
{
    if (out_kernel_ms) *out_kernel_ms = 0.0f;
    if (out) *out = nullptr;
    if (!R || !labels || !pair_masks || !out) return fail(MI_EINVAL, "NULL argument");
    if (m < 1 || m > MI_ANNOT_MAX_GENES) return fail(MI_EUNSUPPORTED, "m must be in [1, %d] (got %d)", MI_ANNOT_MAX_GENES, m);
    if (L < 1 || L > MI_ANNOT_MAX_LABELS) return fail(MI_EUNSUPPORTED, "L must be in [1, %d] (got %d)", MI_ANNOT_MAX_LABELS, L);
    if (S < L || S > MI_ANNOT_MAX_SAMPLES)
        return fail(MI_EUNSUPPORTED, "S must be in [L = %d, %d] (got %d)", L, MI_ANNOT_MAX_SAMPLES, S);
    const int W = (m + 31) / 32;
    mi_annot *h = nullptr;
    const int rc = guarded([&]() -> int {
        std::vector<int32_t> off((size_t)L + 1, 0);
        for (int s = 0; s < S; ++s) {
            if (labels[s] < 0 || labels[s] >= L) return fail(MI_EINVAL, "label %d of sample %d is not in [0, %d)", labels[s], s, L);
            ++off[(size_t)labels[s] + 1];
        }
        for (int l = 0; l < L; ++l) {
            if (off[(size_t)l + 1] == 0) return fail(MI_EINVAL, "label %d has no samples", l);
            off[(size_t)l + 1] += off[l];
        }
        size_t bad = 0;
        if (!finite_bits(R, (size_t)S * m, &bad)) return fail(MI_EINVAL, "R[%zu, %zu] is not finite", bad / m, bad % m);
        if (m % 32) {
            const uint32_t past = ~0u << (m % 32);
            for (size_t r = 0; r < (size_t)L * L; ++r)
                if (pair_masks[r * W + (W - 1)] & past) return fail(MI_EINVAL, "pair mask %zu has a bit at or past m = %d", r, m);
        }
        // the samples grouped by label, each label's in the caller's order
        std::vector<int32_t> at(off.begin(), off.end() - 1), perm((size_t)S);
        std::vector<float> G((size_t)S * m);
        for (int s = 0; s < S; ++s) {
            const int p = at[labels[s]]++;
            perm[p] = s;
            std::copy(R + (size_t)s * m, R + (size_t)(s + 1) * m, G.begin() + (size_t)p * m);
        }
        MI_TRY(pick_device(device));
        h = new mi_annot();
        h->S = S; h->m = m; h->L = L; h->W = W; h->mpad = (m + 63) / 64 * 64; h->device = device;
        h->perm.swap(perm);
        HIP_TRY(hipDeviceGetAttribute(&h->cus, hipDeviceAttributeMultiprocessorCount, device));
        HIP_TRY(h->d_R.upload(G));
        HIP_TRY(h->d_off.upload(off));
        HIP_TRY(h->d_masks.upload(pair_masks, (size_t)L * L * W));
        HIP_TRY(h->d_rhi.resize((size_t)S * h->mpad));
        HIP_TRY(h->d_rlo.resize((size_t)S * h->mpad));
        HIP_TRY(h->d_sb2.resize((size_t)S));
        Timer tm;
        MI_TRY(tm.start(0));
        MI_TRY(launch_rank(h->d_R, S, m, h->mpad, h->d_rhi, h->d_rlo, h->d_sb2));
        MI_TRY(tm.stop(0, out_kernel_ms));
        return MI_OK;
    });
    if (rc != MI_OK) {
        delete h;
        return rc;
    }
    *out = h;
    return MI_OK;
}

int mi_annot_score(mi_annot *h, const float *X, int n_c, int64_t *out_sab, int64_t *out_sa2, int64_t *out_sb2,
                   double *out_scores, int32_t *out_first, float *out_kernel_ms)
{
    if (out_kernel_ms) out_kernel_ms[0] = out_kernel_ms[1] = out_kernel_ms[2] = 0.0f;
    if (!h) return fail(MI_EINVAL, "NULL argument");
    h->n_c = 0;                                // a refused or failed call leaves no resident chunk
    if (!X) return fail(MI_EINVAL, "NULL argument");
    if (n_c < 1) return fail(MI_EINVAL, "n_c must be >= 1 (got %d)", n_c);
    if (n_c > MI_ANNOT_MAX_CHUNK) return fail(MI_EUNSUPPORTED, "%d cells exceed a chunk of %d", n_c, MI_ANNOT_MAX_CHUNK);
    const int m = h->m;
    size_t bad = 0;
    if (!finite_bits(X, (size_t)n_c * m, &bad)) return fail(MI_EINVAL, "X[%zu, %zu] is not finite", bad / m, bad % m);
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(h->device));
        MI_TRY(reserve_chunk(h, n_c));
        HIP_TRY(hipMemcpy(h->d_X, X, (size_t)n_c * m * sizeof(float), hipMemcpyHostToDevice));
        return score_chunk(h, n_c, out_sab, out_sa2, out_sb2, out_scores, out_first, out_kernel_ms);
    });
}

int mi_annot_fine_tune(mi_annot *h, int32_t *out_labels, double *out_best, double *out_next, int32_t *out_iterations,
                       float *out_kernel_ms)
{
    if (out_kernel_ms) *out_kernel_ms = 0.0f;
    if (!h) return fail(MI_EINVAL, "NULL handle");
    if (h->n_c < 1) return fail(MI_ESTATE, "mi_annot_score has not run");
    const int n_c = h->n_c;
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(h->d_labels.reserve((size_t)n_c));
        HIP_TRY(h->d_iters.reserve((size_t)n_c));
        HIP_TRY(h->d_best.reserve((size_t)n_c));
        HIP_TRY(h->d_next.reserve((size_t)n_c));
        TuneArgs a;
        a.X = h->d_X; a.R = h->d_R; a.off = h->d_off; a.masks = h->d_masks; a.scores = h->d_scores;
        a.n = n_c; a.S = h->S; a.L = h->L; a.m = h->m; a.W = h->W; a.mpad = h->mpad; a.cap = sort_cap(h->m);
        a.labels = h->d_labels; a.iters = h->d_iters; a.best = h->d_best; a.next = h->d_next;
        const size_t bytes = tune_lds_bytes(a.cap, a.mpad, a.W, a.S);
        MI_TRY(allow_lds(k_annot_fine_tune, bytes));
        Timer tm;
        MI_TRY(tm.start(0));
        hipLaunchKernelGGL(k_annot_fine_tune, dim3((unsigned)n_c), dim3(kAnnotThreads), bytes, 0, a);
        MI_TRY(tm.stop(0, out_kernel_ms));
        if (out_labels) HIP_TRY(hipMemcpy(out_labels, h->d_labels, (size_t)n_c * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (out_best) HIP_TRY(hipMemcpy(out_best, h->d_best, (size_t)n_c * sizeof(double), hipMemcpyDeviceToHost));
        if (out_next) HIP_TRY(hipMemcpy(out_next, h->d_next, (size_t)n_c * sizeof(double), hipMemcpyDeviceToHost));
        if (out_iterations) HIP_TRY(hipMemcpy(out_iterations, h->d_iters, (size_t)n_c * sizeof(int32_t), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_annot_score_matrix(mi_annot *h, mi_prep_matrix *M, int which, const int32_t *cols, int row0, int n_c, int64_t *out_sab,
                          int64_t *out_sa2, int64_t *out_sb2, double *out_scores, int32_t *out_first, float *out_kernel_ms)
{
    if (out_kernel_ms) out_kernel_ms[0] = out_kernel_ms[1] = out_kernel_ms[2] = out_kernel_ms[3] = 0.0f;
    if (!h) return fail(MI_EINVAL, "NULL argument");
    h->n_c = 0;                                // a refused or failed call leaves no resident chunk
    return guarded([&]() -> int {
        if (!M || !cols) return fail(MI_EINVAL, "NULL argument");
        MI_TRY(check_source(h, M, which));
        if (row0 < 0 || n_c < 1 || (long long)row0 + n_c > M->n)
            return fail(MI_EINVAL, "rows [%d, %d + %d) are not a range of the %d cells", row0, row0, n_c, M->n);
        if (n_c > MI_ANNOT_MAX_CHUNK) return fail(MI_EUNSUPPORTED, "%d cells exceed a chunk of %d", n_c, MI_ANNOT_MAX_CHUNK);
        const int m = h->m;
        std::vector<int32_t> gmap;
        MI_TRY(check_cols(cols, m, M->g, gmap));
        MI_TRY(check_state(M, which == MI_PREP_MARKERS_NORMALIZED ? NEED_NORMALIZED : 0));
        // (the handle's values are finite and non-negative by mi_prep_create*'s checks: no scan)
        HIP_TRY(hipSetDevice(h->device));
        MI_TRY(reserve_chunk(h, n_c));
        const float *V = which == MI_PREP_MARKERS_NORMALIZED ? M->d_Y : M->d_X;
        DevBufs bufs;
        {
            Timer tm;
            if (M->sparse) {
                int32_t *d_gmap = nullptr;
                HIP_TRY(bufs.upload(&d_gmap, gmap.data(), gmap.size()));
                MI_TRY(tm.start(0));
                hipLaunchKernelGGL(k_annot_gather_csr, dim3((unsigned)n_c), dim3(kAnnotThreads), (size_t)m * sizeof(uint32_t), 0,
                                   M->d_indptr, M->d_indices, V, d_gmap, row0, n_c, m, h->d_X);
            } else {
                int32_t *d_cols = nullptr;
                HIP_TRY(bufs.upload(&d_cols, cols, (size_t)m));
                MI_TRY(tm.start(0));
                hipLaunchKernelGGL(k_annot_gather_dense, dim3((unsigned)((m + kAnnotThreads - 1) / kAnnotThreads), (unsigned)n_c),
                                   dim3(kAnnotThreads), 0, 0, V, (long long)M->g, row0, d_cols, n_c, m, h->d_X);
            }
            MI_TRY(tm.stop(0, out_kernel_ms ? out_kernel_ms + 0 : nullptr));
        }
        return score_chunk(h, n_c, out_sab, out_sa2, out_sb2, out_scores, out_first, out_kernel_ms ? out_kernel_ms + 1 : nullptr);
    });
}

int mi_annot_score_clusters(mi_annot *h, mi_prep_matrix *M, int which, const int32_t *cols, const int32_t *cluster_of, int K,
                            int32_t *out_sizes, int64_t *out_sab, int64_t *out_sa2, int64_t *out_sb2, double *out_scores,
                            int32_t *out_first, float *out_kernel_ms)
{
    if (out_kernel_ms) out_kernel_ms[0] = out_kernel_ms[1] = out_kernel_ms[2] = out_kernel_ms[3] = 0.0f;
    if (!h) return fail(MI_EINVAL, "NULL argument");
    h->n_c = 0;                                // a refused or failed call leaves no resident chunk
    return guarded([&]() -> int {
        if (!M || !cols) return fail(MI_EINVAL, "NULL argument");
        MI_TRY(check_source(h, M, which));
        if (!cluster_of) return fail(MI_EINVAL, "NULL argument");
        if (K < 1) return fail(MI_EINVAL, "K must be >= 1 (got %d)", K);
        if (K > MI_ANNOT_MAX_CHUNK) return fail(MI_EUNSUPPORTED, "%d clusters exceed a chunk of %d", K, MI_ANNOT_MAX_CHUNK);
        const int m = h->m, n = M->n;
        std::vector<int32_t> gmap, sizes((size_t)K, 0);
        MI_TRY(check_cols(cols, m, M->g, gmap));
        for (int i = 0; i < n; ++i) {
            if (cluster_of[i] < 0 || cluster_of[i] >= K)
                return fail(MI_EINVAL, "cluster %d of cell %d is not in [0, %d)", cluster_of[i], i, K);
            ++sizes[cluster_of[i]];
        }
        for (int c = 0; c < K; ++c)
            if (sizes[c] == 0) return fail(MI_EINVAL, "cluster %d has no cells", c);
        MI_TRY(check_state(M, which == MI_PREP_MARKERS_NORMALIZED ? NEED_NORMALIZED : 0));
        HIP_TRY(hipSetDevice(h->device));
        MI_TRY(reserve_chunk(h, K));
        const float *V = which == MI_PREP_MARKERS_NORMALIZED ? M->d_Y : M->d_X;
        DevBufs bufs;
        int32_t *d_cols = nullptr, *d_of = nullptr, *d_sizes = nullptr;
        HIP_TRY(bufs.upload(&d_cols, cols, (size_t)m));
        HIP_TRY(bufs.upload(&d_of, cluster_of, (size_t)n));
        HIP_TRY(bufs.upload(&d_sizes, sizes.data(), sizes.size()));
        {
            const dim3 grid((unsigned)((m + kAnnotWaves - 1) / kAnnotWaves), (unsigned)((K + 63) / 64));
            Timer tm;
            MI_TRY(tm.start(0));
            if (M->sparse) {
                CscColumn src;
                src.colptr = M->d_colptr; src.rows = M->d_rows; src.pos = M->d_pos; src.V = V;
                hipLaunchKernelGGL(k_annot_means<CscColumn>, grid, dim3(kAnnotThreads), 0, 0, src, d_cols, d_of, d_sizes, K, m, h->d_X);
            } else {
                DenseColumn src;
                src.V = V; src.n = n; src.g = M->g;
                hipLaunchKernelGGL(k_annot_means<DenseColumn>, grid, dim3(kAnnotThreads), 0, 0, src, d_cols, d_of, d_sizes, K, m, h->d_X);
            }
            MI_TRY(tm.stop(0, out_kernel_ms ? out_kernel_ms + 0 : nullptr));
        }
        if (out_sizes) std::copy(sizes.begin(), sizes.end(), out_sizes);
        return score_chunk(h, K, out_sab, out_sa2, out_sb2, out_scores, out_first, out_kernel_ms ? out_kernel_ms + 1 : nullptr);
    });
}

int mi_annot_fetch_chunk(mi_annot *h, float *out)
{
    if (!h || !out) return fail(MI_EINVAL, "NULL argument");
    if (h->n_c < 1) return fail(MI_ESTATE, "no chunk is resident");
    return guarded([&]() -> int {
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipMemcpy(out, h->d_X, (size_t)h->n_c * h->m * sizeof(float), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

}  // extern "C"
