// markers_kernels.hip -- batched Wilcoxon rank-sum statistics per (labelling, gene, cluster) (gfx950).
// C ABI: include/mi_metrics.h (mi_rank_sum_markers_f32); the closed forms (U, p, log fold change) are host fp64 in metrics.py.
//
// X is n cells x g genes, L is B labellings of the n cells.  A gene's ranks do not depend on the labelling, so a gene is
// sorted once and scored against every labelling.  Its zeros (both signs) are one tie block whose rank is known without a
// sort: with `neg` negative and `zeros` zero cells the block holds the ranks neg + 1 .. neg + zeros.
//
//   k_markers_transpose  64 x 64 tiles through LDS (row padded by one float): X -> gene-major Xt, coalesced on both sides.
//   k_markers_rank       one workgroup per gene, grid-stride.  The gene's non-zeros are sorted as (key << 32 | cell) and
//                        every sorted position gets its doubled midrank and its tie run by mi_midrank.h (wg_midranks).
//                        The labellings are then scored kMarkersChunk at a time: per (labelling, cluster) one 64-bit LDS
//                        word takes the doubled midranks (bits 0 .. 41: the sum over all n cells is n (n + 1) < 2^42 for
//                        n <= 2^20) and the number of non-zero cells (bits 42 .. 62) in ONE integer atomic per (entry,
//                        labelling); negative entries, rare, are counted in a second word.  The zero block's share is
//                        (cluster size - its non-zero cells) * (2 neg + zeros + 1).  The sorted array and the midranks
//                        live in LDS when the gene's non-zero count fits the launch's LDS plan, else in the workgroup's
//                        slab in HBM (same code; barriers order the slab's accesses inside the workgroup).
//   k_markers_sums       one thread per (gene, labelling), labelling fastest: walks the cells in ascending order and adds
//                        expm1((double)x), or (double)x, to the private accumulator of the cell's cluster (LDS, one column
//                        per thread).  A zero adds nothing (+0.0 + -0.0 = +0.0), so it is skipped; with many labellings a
//                        wavefront shares its gene and skips the zero as one.
//
// mi_prep_rank_sum_markers (include/mi_prep.h) runs the same pass on a resident mi_prep_matrix.  A dense handle hands its
// device matrix to the three kernels above (k_markers_count gives the per-gene non-zero counts the host scan gives the
// host entry).  A sparse handle has the genes' stored entries already gene-major (colptr, rows, pos): no transpose and no
// n x g buffer.  rank_gene is one body for both: it is a template on how a gene's candidates are enumerated (DenseGenes:
// the n cells of Xt's row; CscGenes: the stored entries, cell = rows[k], value = V[pos[k]]).  The launch is planned from
// an upper bound of each gene's non-zeros (the stored count; exact for a dense matrix); the compaction skips stored zeros
// and yields the true count, which everything after it uses, the sort's power of two included.
//   k_markers_permute    Vg[k] = V[pos[k]]: the values in gene-major order, nnz floats of scratch (one of the two gather forms)
//   k_markers_sums_csc   k_markers_sums on the stored entries: the same additions in the same (ascending cell) order, so the
//                        sums are bit for bit the dense kernel's.
// Integer atomics only; stores are ordinary vector stores.
#include <vector>

#include "../../include/mi_metrics.h"
#include "../../include/mi_prep.h"
#include "mi_markers_plan.h"
#include "mi_midrank.h"
#include "mi_prep_handle.h"
#include "mi_sa_device.h"

namespace mi_sa_impl {
namespace {

constexpr int kMarkersChunk = MI_MARKERS_LABELLING_CHUNK;
constexpr int kMarkersTile = 64;
constexpr int kSumThreads = 128;
constexpr int kRankBits = 42;                                                            // n (n + 1) < 2^42 for n <= 2^20
constexpr unsigned long long kRankMask = (1ull << kRankBits) - 1ull;
constexpr size_t kSlabBudget = (size_t)1 << 30;                                          // bytes of HBM for all slabs
constexpr bool kPermuteByDefault = true;                                                 // a sparse handle's value gather (profiles/markers_sparse.json)

struct MarkersArgs {
    const uint16_t *Lt = nullptr;          // n x Bp, cell-major labels (rows padded to Bp)
    const int32_t *sizes = nullptr;        // B x K cluster sizes
    int n = 0, g = 0, B = 0, Bp = 0, K = 0;
    int lds_cap = 0;                       // entries of the LDS arrays (a power of two, or 0)
    unsigned long long *slab = nullptr;    // gridDim.x x slab_stride sorted entries in HBM
    uint32_t *slab_mid = nullptr;          // ... and their doubled midranks
    size_t slab_stride = 0;
    long long *rank2 = nullptr;            // B x g x K
    int32_t *npos = nullptr;               // B x g x K
    long long *tie = nullptr;              // g
};

using mi_midrank::zero_bits;

__global__ void __launch_bounds__(256) k_markers_transpose(const float *__restrict__ X, float *__restrict__ Xt, int n, int g)
{
    __shared__ float tile[kMarkersTile][kMarkersTile + 1];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const size_t j0 = (size_t)blockIdx.x * kMarkersTile, i0 = (size_t)blockIdx.y * kMarkersTile;
    for (int r = ty; r < kMarkersTile; r += 4) {
        const size_t i = i0 + r, j = j0 + tx;
        if (i < (size_t)n && j < (size_t)g) tile[r][tx] = X[i * g + j];
    }
    __syncthreads();
    for (int r = ty; r < kMarkersTile; r += 4) {
        const size_t j = j0 + r, i = i0 + tx;
        if (i < (size_t)n && j < (size_t)g) Xt[j * n + i] = tile[tx][r];
    }
}

// How a gene's candidates (the cells that may hold a non-zero) are enumerated: candidate i of `count` has the cell
// cell(i), ascending in i, and the value bits(i).  planned(): the upper bound of the gene's non-zeros the launch was
// planned with.
struct DenseGenes {                        // the n cells of row `gene` of Xt (g x n)
    const float *Xt = nullptr;
    const int32_t *nnz = nullptr;          // g non-zero cells per gene (exact)
    int n = 0;
    struct Gene {
        const float *row;
        int count;
        __device__ __forceinline__ uint32_t bits(int i) const { return __float_as_uint(row[i]); }
        __device__ __forceinline__ uint32_t cell(int i) const { return (uint32_t)i; }
    };
    __device__ __forceinline__ Gene gene(int j) const { return Gene{Xt + (size_t)j * n, n}; }
    __device__ __forceinline__ int planned(int j) const { return nnz[j]; }
};

struct CscGenes {                          // the stored entries colptr[gene] .. colptr[gene + 1] - 1 of a sparse handle
    const int64_t *colptr = nullptr;
    const int32_t *rows = nullptr;
    const int32_t *pos = nullptr;          // entry k has the value V[pos[k]]; nullptr: V is gene-major already, V[k]
    const float *V = nullptr;
    struct Gene {
        const int32_t *rows, *pos;
        const float *V;
        int count;
        __device__ __forceinline__ uint32_t bits(int i) const { return __float_as_uint(pos ? V[pos[i]] : V[i]); }
        __device__ __forceinline__ uint32_t cell(int i) const { return (uint32_t)rows[i]; }
    };
    __device__ __forceinline__ Gene gene(int j) const
    {
        const int64_t k0 = colptr[j];
        return Gene{rows + k0, pos ? pos + k0 : nullptr, pos ? V : V + k0, (int)(colptr[j + 1] - k0)};
    }
    __device__ __forceinline__ int planned(int j) const { return (int)(colptr[j + 1] - colptr[j]); }
};

// One gene, whole workgroup.  S (`cap` entries, a power of two >= the gene's planned count) and mid (as many entries as
// there are non-zeros) are in LDS or in HBM.
template <class Src>
__device__ __forceinline__ void rank_gene(const MarkersArgs &a, const Src &src, int gene, int cap, unsigned long long *S,
                                          uint32_t *mid, unsigned long long *acc, uint32_t *negc, unsigned long long *s_tie,
                                          uint32_t *s_cnt)
{
    const int K = a.K, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    if (tid == 0) *s_tie = 0ull;                                                         // (published by wg_midranks' first barrier)

    // doubled midrank of every sorted position, with the sign of its value; tie term of the non-zero runs
    const typename Src::Gene cand = src.gene(gene);
    long long tie = 0;
    const mi_midrank::Ranked rk = mi_midrank::wg_midranks(
        cand.count, [&](int i) { return cand.bits(i); }, [&](int i) { return cand.cell(i); }, a.n, cap, S, s_cnt,
        [&](int p, unsigned long long e, int lo, int hi, uint32_t r2) {
            mid[p] = r2 | ((e >> 63) ? 0u : 0x80000000u);
            if (lo == p) {
                const long long t = hi - lo;
                tie += t * t * t - t;
            }
        });
    const int nnz = rk.nnz;
    for (int off = 32; off > 0; off >>= 1) tie += __shfl_xor(tie, off);
    if (lane == 0 && tie) atomicAdd(s_tie, (unsigned long long)tie);
    __syncthreads();
    if (tid == 0 && a.tie) {
        const long long z = rk.zeros;
        a.tie[gene] = (long long)*s_tie + z * z * z - z;
    }

    const long long zmid2 = rk.zero_r2;
    for (int b0 = 0; b0 < a.B; b0 += kMarkersChunk) {
        const int nb = a.B - b0 < kMarkersChunk ? a.B - b0 : kMarkersChunk;
        for (int t = tid; t < nb * K; t += nt) {
            acc[t] = 0ull;
            negc[t] = 0u;
        }
        __syncthreads();
        for (int p = tid; p < nnz; p += nt) {
            const uint32_t cell = (uint32_t)S[p], m = mid[p];
            const unsigned long long add = (unsigned long long)(m & 0x7fffffffu) | (1ull << kRankBits);
            const uint16_t *lab = a.Lt + (size_t)cell * a.Bp + b0;
            for (int bb = 0; bb < nb; ++bb) {
                const int c = lab[bb];
                atomicAdd(&acc[bb * K + c], add);
                if (m >> 31) atomicAdd(&negc[bb * K + c], 1u);
            }
        }
        __syncthreads();
        for (int t = tid; t < nb * K; t += nt) {
            const int bb = t / K, c = t - bb * K;
            const unsigned long long v = acc[t];
            const long long nzc = (long long)(v >> kRankBits);
            const size_t o = ((size_t)(b0 + bb) * a.g + gene) * K + c;
            a.rank2[o] = (long long)(v & kRankMask) + ((long long)a.sizes[(size_t)(b0 + bb) * K + c] - nzc) * zmid2;
            a.npos[o] = (int32_t)(nzc - (long long)negc[t]);
        }
        __syncthreads();                                                                 // (acc is cleared by the next chunk, s_* by the next gene)
    }
}

template <class Src>
__global__ void __launch_bounds__(1024) k_markers_rank(MarkersArgs a, Src src)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ unsigned long long s_tie;
    __shared__ uint32_t s_cnt[2];
    unsigned long long *S = reinterpret_cast<unsigned long long *>(lds);
    uint32_t *mid = reinterpret_cast<uint32_t *>(lds + (size_t)a.lds_cap * 8);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(lds + (size_t)a.lds_cap * 12);
    uint32_t *negc = reinterpret_cast<uint32_t *>(acc + kMarkersChunk * a.K);
    for (int gene = blockIdx.x; gene < a.g; gene += gridDim.x) {
        if (src.planned(gene) <= a.lds_cap) rank_gene(a, src, gene, a.lds_cap, S, mid, acc, negc, &s_tie, s_cnt);
        else rank_gene(a, src, gene, (int)a.slab_stride, a.slab + blockIdx.x * a.slab_stride, a.slab_mid + blockIdx.x * a.slab_stride, acc, negc, &s_tie, s_cnt);
    }
}

// per-gene non-zero cells of a row-major device matrix: 64 genes x 4 row lanes per workgroup over a slice of rows
constexpr int kCountSlice = 256;
__global__ void __launch_bounds__(256) k_markers_count(const float *__restrict__ X, int n, int g, int32_t *__restrict__ nnz)
{
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const size_t j = (size_t)blockIdx.x * 64 + tx;
    const int r0 = (int)blockIdx.y * kCountSlice, r1 = r0 + kCountSlice < n ? r0 + kCountSlice : n;
    if (j >= (size_t)g) return;
    int cnt = 0;
    for (int i = r0 + ty; i < r1; i += 4) cnt += !zero_bits(__float_as_uint(X[(size_t)i * g + j]));
    if (cnt) atomicAdd(&nnz[j], cnt);
}

__global__ void __launch_bounds__(256) k_markers_permute(const float *__restrict__ V, const int32_t *__restrict__ pos,
                                                         size_t nnz, float *__restrict__ Vg)
{
    for (size_t k = (size_t)blockIdx.x * 256 + threadIdx.x; k < nnz; k += (size_t)gridDim.x * 256) Vg[k] = V[pos[k]];
}

// M[i * si + gene * sg]: X itself (si = g, sg = 1: neighbouring genes coalesce) or Xt (si = 1, sg = n: a wavefront that
// shares one gene reads along its row)
__global__ void __launch_bounds__(kSumThreads) k_markers_sums(const float *__restrict__ M, size_t si, size_t sg,
                                                              const uint16_t *__restrict__ Lt, int n, int g, int B, int Bp,
                                                              int K, int plain, double *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    double *acc = reinterpret_cast<double *>(lds) + threadIdx.x;                         // acc[c * kSumThreads]: this thread's column
    const size_t t = (size_t)blockIdx.x * kSumThreads + threadIdx.x;
    if (t >= (size_t)g * B) return;
    const size_t gene = t / B;
    const int b = (int)(t - gene * B);
    for (int c = 0; c < K; ++c) acc[c * kSumThreads] = 0.0;
    const float *x = M + gene * sg;
    const uint16_t *lab = Lt + b;
    for (int i = 0; i < n; ++i) {
        const float v = x[(size_t)i * si];
        if (zero_bits(__float_as_uint(v))) continue;
        const int c = lab[(size_t)i * Bp];
        acc[c * kSumThreads] += plain ? (double)v : expm1((double)v);
    }
    for (int c = 0; c < K; ++c) out[((size_t)b * g + gene) * K + c] = acc[c * kSumThreads];
}

// the same thread, accumulators and additions over the gene's stored entries (cells ascending; a stored zero is skipped as
// the dense kernel skips every zero)
__global__ void __launch_bounds__(kSumThreads) k_markers_sums_csc(CscGenes src, const uint16_t *__restrict__ Lt, int g, int B,
                                                                  int Bp, int K, int plain, double *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    double *acc = reinterpret_cast<double *>(lds) + threadIdx.x;
    const size_t t = (size_t)blockIdx.x * kSumThreads + threadIdx.x;
    if (t >= (size_t)g * B) return;
    const size_t gene = t / B;
    const int b = (int)(t - gene * B);
    for (int c = 0; c < K; ++c) acc[c * kSumThreads] = 0.0;
    const CscGenes::Gene cand = src.gene((int)gene);
    const uint16_t *lab = Lt + b;
    for (int k = 0; k < cand.count; ++k) {
        const uint32_t u = cand.bits(k);
        if (zero_bits(u)) continue;
        const float v = __uint_as_float(u);
        const int c = lab[(size_t)cand.cell(k) * Bp];
        acc[c * kSumThreads] += plain ? (double)v : expm1((double)v);
    }
    for (int c = 0; c < K; ++c) out[((size_t)b * g + gene) * K + c] = acc[c * kSumThreads];
}

// what an entry point asks for: the shape, the labellings and the caller's outputs (host pointers)
struct MarkersCall {
    int n = 0, g = 0, B = 0, K = 0;
    uint32_t flags = 0;
    const uint16_t *L = nullptr;
    int64_t *out_rank2 = nullptr;
    int32_t *out_npos = nullptr;
    double *out_sum = nullptr;
    int64_t *out_tie = nullptr;
    int Bp() const { return (B + kMarkersChunk - 1) / kMarkersChunk * kMarkersChunk; }
    size_t entries() const { return (size_t)B * g * K; }
};

// the checks both entry points make of B, K, the flags (`known`: the bits the entry accepts) and the output cap
int check_call(const MarkersCall &c, uint32_t known)
{
    if (c.B < 1) return fail(MI_EINVAL, "B must be >= 1 (got %d)", c.B);
    if (c.K < 1 || c.K > 64) return fail(MI_EINVAL, "K must be in [1, 64] (got %d)", c.K);
    if (c.flags & ~known) return fail(MI_EINVAL, "unknown flags 0x%x", c.flags);
    return MI_OK;
}

int check_limits(const MarkersCall &c)
{
    if (c.n > MI_MARKERS_MAX_CELLS) return fail(MI_EUNSUPPORTED, "%d cells exceed %d", c.n, MI_MARKERS_MAX_CELLS);
    if ((double)c.B * (double)c.g * (double)c.K > (double)MI_MARKERS_MAX_ENTRIES)
        return fail(MI_EUNSUPPORTED, "%d labellings x %d genes x %d clusters exceed %lld output entries", c.B, c.g, c.K,
                    (long long)MI_MARKERS_MAX_ENTRIES);
    return MI_OK;
}

// host scan of the labels: range, cluster sizes (B x K), cell-major copy (n x Bp)
int scan_labels(const MarkersCall &c, std::vector<int32_t> &sizes, std::vector<uint16_t> &Lt)
{
    const int Bp = c.Bp();
    sizes.assign((size_t)c.B * c.K, 0);
    Lt.assign((size_t)c.n * Bp, 0);
    for (int b = 0; b < c.B; ++b)
        for (int i = 0; i < c.n; ++i) {
            const uint16_t l = c.L[(size_t)b * c.n + i];
            if (l >= c.K) return fail(MI_EINVAL, "label %d of labelling %d, cell %d is not below K = %d", (int)l, b, i, c.K);
            ++sizes[(size_t)b * c.K + l];
            Lt[(size_t)i * Bp + b] = l;
        }
    return MI_OK;
}

// The launch half of a call, on device pointers: the plan from the genes' planned counts, the scratch (owned by `bufs`),
// the ranking pass over any source of candidates, and the copies out.  The current device is the caller's business.
struct MarkersRun {
    MarkersArgs a;
    uint16_t *d_Lt = nullptr;
    double *d_sum = nullptr;
    size_t lds_bytes = 0, grid = 1;
    int threads = 256;

    // counts: g planned non-zero counts (host).  The plan (mi_markers_plan.h): the LDS arrays hold the largest count at or
    // below the cap, the slabs the largest above.
    int prepare(DevBufs &bufs, const MarkersCall &c, const std::vector<int32_t> &sizes, const std::vector<uint16_t> &Lt,
                const int32_t *counts, int device)
    {
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        const mi_markers_plan::Plan p = mi_markers_plan::plan(counts, c.g, c.K, (c.flags & MI_MARKERS_GLOBAL) ? 0 : MI_MARKERS_LDS_MAX_NONZEROS,
                                                              kMarkersChunk, cus, kSlabBudget);
        const int lds_cap = p.lds_cap;
        const size_t slab_stride = p.slab_stride;
        lds_bytes = p.lds_bytes;
        threads = p.threads;
        grid = p.grid;

        int32_t *d_sizes = nullptr, *d_npos = nullptr;
        long long *d_rank2 = nullptr, *d_tie = nullptr;
        unsigned long long *d_slab = nullptr;
        uint32_t *d_slab_mid = nullptr;
        const size_t entries = c.entries();
        HIP_TRY(bufs.upload(&d_Lt, Lt.data(), Lt.size()));
        HIP_TRY(bufs.upload(&d_sizes, sizes.data(), sizes.size()));
        HIP_TRY(bufs.alloc(&d_rank2, entries));
        HIP_TRY(bufs.alloc(&d_npos, entries));
        HIP_TRY(bufs.alloc(&d_tie, (size_t)c.g));
        if (c.out_sum) HIP_TRY(bufs.alloc(&d_sum, entries));
        if (slab_stride) {
            HIP_TRY(bufs.alloc(&d_slab, grid * slab_stride));
            HIP_TRY(bufs.alloc(&d_slab_mid, grid * slab_stride));
        }

        a.Lt = d_Lt; a.sizes = d_sizes;
        a.n = c.n; a.g = c.g; a.B = c.B; a.Bp = c.Bp(); a.K = c.K; a.lds_cap = lds_cap;
        a.slab = d_slab; a.slab_mid = d_slab_mid; a.slab_stride = slab_stride;
        a.rank2 = d_rank2; a.npos = d_npos; a.tie = d_tie;
        return MI_OK;
    }

    template <class Src>
    int rank(const Src &src)
    {
        MI_TRY(allow_lds(k_markers_rank<Src>, lds_bytes));
        hipLaunchKernelGGL(k_markers_rank<Src>, dim3((unsigned)grid), dim3((unsigned)threads), lds_bytes, 0, a, src);
        HIP_TRY(hipGetLastError());
        return MI_OK;
    }

    unsigned sum_blocks() const { return (unsigned)(((size_t)a.g * a.B + kSumThreads - 1) / kSumThreads); }
    size_t sum_lds() const { return (size_t)a.K * kSumThreads * sizeof(double); }

    // transpose, rank, sums on a row-major device matrix X (n x g) and its scratch Xt; d_nnz: the exact counts
    int run_dense(const MarkersCall &c, const float *d_X, float *d_Xt, const int32_t *d_nnz)
    {
        hipLaunchKernelGGL(k_markers_transpose, dim3((unsigned)((c.g + kMarkersTile - 1) / kMarkersTile), (unsigned)((c.n + kMarkersTile - 1) / kMarkersTile)),
                           dim3(256), 0, 0, d_X, d_Xt, c.n, c.g);
        HIP_TRY(hipGetLastError());
        DenseGenes src;
        src.Xt = d_Xt; src.nnz = d_nnz; src.n = c.n;
        MI_TRY(rank(src));
        if (c.out_sum) {
            // a wavefront holds 64 / B genes: with few labellings neighbouring genes coalesce in X, with many it reads Xt's row
            const bool rows = c.B >= kMarkersChunk;
            hipLaunchKernelGGL(k_markers_sums, dim3(sum_blocks()), dim3(kSumThreads), sum_lds(), 0, rows ? d_Xt : d_X,
                               rows ? (size_t)1 : (size_t)c.g, rows ? (size_t)c.n : (size_t)1, d_Lt, c.n, c.g, c.B, a.Bp, c.K,
                               (c.flags & MI_MARKERS_SUM_PLAIN) ? 1 : 0, d_sum);
            HIP_TRY(hipGetLastError());
        }
        return MI_OK;
    }

    // rank, sums on the stored entries; d_Vg: nnz floats of scratch for the gene-major values, or nullptr to gather in place
    int run_csc(const MarkersCall &c, CscGenes src, size_t nnz, float *d_Vg)
    {
        if (d_Vg) {
            if (nnz) {
                const size_t blocks = (nnz + 255) / 256;
                hipLaunchKernelGGL(k_markers_permute, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, 0, src.V, src.pos,
                                   nnz, d_Vg);
                HIP_TRY(hipGetLastError());
            }
            src.V = d_Vg;
            src.pos = nullptr;
        }
        MI_TRY(rank(src));
        if (c.out_sum) {
            hipLaunchKernelGGL(k_markers_sums_csc, dim3(sum_blocks()), dim3(kSumThreads), sum_lds(), 0, src, d_Lt, c.g, c.B, a.Bp,
                               c.K, (c.flags & MI_MARKERS_SUM_PLAIN) ? 1 : 0, d_sum);
            HIP_TRY(hipGetLastError());
        }
        return MI_OK;
    }

    int fetch(const MarkersCall &c)
    {
        const size_t entries = c.entries();
        HIP_TRY(hipMemcpy(c.out_rank2, a.rank2, entries * sizeof(long long), hipMemcpyDeviceToHost));
        if (c.out_npos) HIP_TRY(hipMemcpy(c.out_npos, a.npos, entries * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (c.out_sum) HIP_TRY(hipMemcpy(c.out_sum, d_sum, entries * sizeof(double), hipMemcpyDeviceToHost));
        if (c.out_tie) HIP_TRY(hipMemcpy(c.out_tie, a.tie, (size_t)c.g * sizeof(long long), hipMemcpyDeviceToHost));
        return MI_OK;
    }
};

}  // namespace
}  // namespace mi_sa_impl
using namespace mi_sa_impl;

extern "C" int mi_rank_sum_markers_f32(const float *X, int n, int g, const uint16_t *L, int B, int K, int device,
                                       uint32_t flags, int64_t *out_rank2, int32_t *out_npos, double *out_sum,
                                       int64_t *out_tie, float *out_kernel_ms)
{
    if (out_kernel_ms) *out_kernel_ms = 0.0f;
    if (!X || !L || !out_rank2) return fail(MI_EINVAL, "NULL argument");
    if (n < 1) return fail(MI_EINVAL, "n must be >= 1 (got %d)", n);
    if (g < 1) return fail(MI_EINVAL, "g must be >= 1 (got %d)", g);
    MarkersCall c;
    c.n = n; c.g = g; c.B = B; c.K = K; c.flags = flags; c.L = L;
    c.out_rank2 = out_rank2; c.out_npos = out_npos; c.out_sum = out_sum; c.out_tie = out_tie;
    MI_TRY(check_call(c, MI_MARKERS_SUM_PLAIN | MI_MARKERS_GLOBAL));
    MI_TRY(check_limits(c));
    return guarded([&]() -> int {
        DevBufs bufs;
        // host scans: the labels (range, cluster sizes, cell-major copy) and X (finite; non-zero cells per gene)
        std::vector<int32_t> sizes, nnz((size_t)g, 0);
        std::vector<uint16_t> Lt;
        MI_TRY(scan_labels(c, sizes, Lt));
        const uint32_t *U = reinterpret_cast<const uint32_t *>(X);
        for (int i = 0; i < n; ++i) {
            const uint32_t *row = U + (size_t)i * g;
            for (int j = 0; j < g; ++j) {
                const uint32_t u = row[j];
                if ((u & 0x7f800000u) == 0x7f800000u) return fail(MI_EINVAL, "X[%d, %d] is not finite", i, j);
                nnz[j] += (u & 0x7fffffffu) != 0u;
            }
        }
        MI_TRY(pick_device(device));
        MarkersRun run;
        float *d_X = nullptr, *d_Xt = nullptr;
        int32_t *d_nnz = nullptr;
        const size_t cells = (size_t)n * g;
        HIP_TRY(bufs.upload(&d_X, X, cells));
        HIP_TRY(bufs.alloc(&d_Xt, cells));
        HIP_TRY(bufs.upload(&d_nnz, nnz.data(), nnz.size()));
        MI_TRY(run.prepare(bufs, c, sizes, Lt, nnz.data(), device));
        Timer tm;
        MI_TRY(tm.start(0));
        MI_TRY(run.run_dense(c, d_X, d_Xt, d_nnz));
        MI_TRY(tm.stop(0, out_kernel_ms));
        return run.fetch(c);
    });
}

extern "C" int mi_prep_rank_sum_markers(mi_prep_matrix *m, int which, const uint16_t *L, int B, int K, uint32_t flags,
                                        int64_t *out_rank2, int32_t *out_npos, double *out_sum, int64_t *out_tie,
                                        float *out_kernel_ms)
{
    return on_matrix(m, L && out_rank2, 0, out_kernel_ms, [&]() -> int {
        if (which != MI_PREP_MARKERS_COUNTS && which != MI_PREP_MARKERS_NORMALIZED)
            return fail(MI_EINVAL, "which must be 0 (counts) or 1 (normalised), got %d", which);
        MarkersCall c;
        c.n = m->n; c.g = m->g; c.B = B; c.K = K; c.flags = flags; c.L = L;
        c.out_rank2 = out_rank2; c.out_npos = out_npos; c.out_sum = out_sum; c.out_tie = out_tie;
        const uint32_t gather = MI_PREP_MARKERS_GATHER_INPLACE | MI_PREP_MARKERS_GATHER_PERMUTE;
        MI_TRY(check_call(c, MI_MARKERS_SUM_PLAIN | MI_MARKERS_GLOBAL | gather));
        if ((flags & gather) == gather) return fail(MI_EINVAL, "flags 0x%x ask for both gather forms", flags);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < c.n; ++i)
                if (L[(size_t)b * c.n + i] >= K)
                    return fail(MI_EINVAL, "label %d of labelling %d, cell %d is not below K = %d", (int)L[(size_t)b * c.n + i], b, i, K);
        MI_TRY(check_state(m, which == MI_PREP_MARKERS_NORMALIZED ? NEED_NORMALIZED : 0));
        MI_TRY(check_limits(c));
        c.flags = flags & ~gather;
        const bool permute = (flags & gather) ? (flags & MI_PREP_MARKERS_GATHER_PERMUTE) != 0 : kPermuteByDefault;
        DevBufs bufs;
        std::vector<int32_t> sizes, counts((size_t)c.g, 0);
        std::vector<uint16_t> Lt;
        MI_TRY(scan_labels(c, sizes, Lt));
        const float *M = which == MI_PREP_MARKERS_NORMALIZED ? m->d_Y : m->d_X;
        MarkersRun run;
        float ms_count = 0.0f, ms = 0.0f;
        if (m->sparse) {
            // the plan comes from the stored counts (an upper bound of the non-zeros), read from the handle's colptr
            std::vector<int64_t> colptr((size_t)c.g + 1);
            HIP_TRY(hipMemcpy(colptr.data(), m->d_colptr, colptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
            mi_markers_plan::stored_counts(colptr.data(), c.g, counts.data());
            float *d_Vg = nullptr;
            if (permute) HIP_TRY(bufs.alloc(&d_Vg, (size_t)m->nnz));
            MI_TRY(run.prepare(bufs, c, sizes, Lt, counts.data(), m->device));
            CscGenes src;
            src.colptr = m->d_colptr; src.rows = m->d_rows; src.pos = m->d_pos; src.V = M;
            Timer tm;
            MI_TRY(tm.start(0));
            MI_TRY(run.run_csc(c, src, (size_t)m->nnz, d_Vg));
            MI_TRY(tm.stop(0, &ms));
        } else {
            // the handle's values are finite and non-negative (mi_prep_create_f32): only the counts are left of the host scan
            float *d_Xt = nullptr;
            int32_t *d_nnz = nullptr;
            HIP_TRY(bufs.alloc(&d_Xt, (size_t)c.n * c.g));
            HIP_TRY(bufs.alloc(&d_nnz, (size_t)c.g));
            HIP_TRY(hipMemset(d_nnz, 0, (size_t)c.g * sizeof(int32_t)));
            {
                Timer tc;
                MI_TRY(tc.start(0));
                hipLaunchKernelGGL(k_markers_count, dim3((unsigned)((c.g + 63) / 64), (unsigned)((c.n + kCountSlice - 1) / kCountSlice)),
                                   dim3(256), 0, 0, M, c.n, c.g, d_nnz);
                MI_TRY(tc.stop(0, &ms_count));
            }
            HIP_TRY(hipMemcpy(counts.data(), d_nnz, counts.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            MI_TRY(run.prepare(bufs, c, sizes, Lt, counts.data(), m->device));
            Timer tm;
            MI_TRY(tm.start(0));
            MI_TRY(run.run_dense(c, M, d_Xt, d_nnz));
            MI_TRY(tm.stop(0, &ms));
        }
        if (out_kernel_ms) *out_kernel_ms = ms_count + ms;
        return run.fetch(c);
    });
}
