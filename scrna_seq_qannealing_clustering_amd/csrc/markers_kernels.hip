// markers_kernels.hip -- batched Wilcoxon rank-sum statistics per (labelling, gene, cluster) (gfx950).
// C ABI: include/mi_metrics.h (mi_rank_sum_markers_f32); the closed forms (U, p, log fold change) are host fp64 in metrics.py.
//
// X is n cells x g genes, L is B labellings of the n cells.  A gene's ranks do not depend on the labelling, so a gene is
// sorted once and scored against every labelling.  Its zeros (both signs) are one tie block whose rank is known without a
// sort: with `neg` negative and `zeros` zero cells the block holds the ranks neg + 1 .. neg + zeros.
//
//   k_markers_transpose  64 x 64 tiles through LDS (row padded by one float): X -> gene-major Xt, coalesced on both sides.
//   k_markers_rank       one workgroup per gene, grid-stride.  The gene's non-zeros are compacted as
//                        (order-preserving u32 key << 32 | cell) -- unique 64-bit words, so the sorted array does not depend
//                        on the order the compaction wrote them in -- padded with ~0 to a power of two and sorted by a
//                        bitonic network.  A sorted position finds its tie run [lo, hi) by its neighbours and, inside a
//                        run, by binary search; its doubled midrank is lo + 1 + hi, plus 2 * zeros for a positive value.
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
// Integer atomics only; stores are ordinary vector stores.
#include <vector>

#include "../../include/mi_metrics.h"
#include "mi_sa_device.h"

namespace mi_sa_impl {
namespace {

constexpr int kMarkersChunk = MI_MARKERS_LABELLING_CHUNK;
constexpr int kMarkersTile = 64;
constexpr int kSumThreads = 128;
constexpr int kRankBits = 42;                                                            // n (n + 1) < 2^42 for n <= 2^20
constexpr unsigned long long kRankMask = (1ull << kRankBits) - 1ull;
constexpr size_t kSlabBudget = (size_t)1 << 30;                                          // bytes of HBM for all slabs

struct MarkersArgs {
    const float *Xt = nullptr;             // g x n
    const uint16_t *Lt = nullptr;          // n x Bp, cell-major labels (rows padded to Bp)
    const int32_t *sizes = nullptr;        // B x K cluster sizes
    const int32_t *nnz = nullptr;          // g non-zero cells per gene
    int n = 0, g = 0, B = 0, Bp = 0, K = 0;
    int lds_cap = 0;                       // entries of the LDS arrays (a power of two, or 0)
    unsigned long long *slab = nullptr;    // gridDim.x x slab_stride sorted entries in HBM
    uint32_t *slab_mid = nullptr;          // ... and their doubled midranks
    size_t slab_stride = 0;
    long long *rank2 = nullptr;            // B x g x K
    int32_t *npos = nullptr;               // B x g x K
    long long *tie = nullptr;              // g
};

__device__ __forceinline__ bool zero_bits(uint32_t u) { return (u & 0x7fffffffu) == 0u; }

// ascending u32 order == ascending float order over the finite non-zero values (equal floats <=> equal keys)
__device__ __forceinline__ uint32_t order_key(uint32_t u) { return (u >> 31) ? ~u : (u | 0x80000000u); }

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

// One gene, whole workgroup.  S (P entries, P = next power of two of nnz) and mid (nnz entries) are in LDS or in HBM.
__device__ __forceinline__ void rank_gene(const MarkersArgs &a, int gene, int nnz, unsigned long long *S, uint32_t *mid,
                                          unsigned long long *acc, uint32_t *negc, unsigned long long *s_tie, uint32_t *s_cnt)
{
    const int n = a.n, K = a.K, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    int P = 0;
    if (nnz > 0)
        for (P = 1; P < nnz; P <<= 1) {}
    if (tid == 0) {
        s_cnt[0] = 0u;
        s_cnt[1] = 0u;
        *s_tie = 0ull;
    }
    __syncthreads();

    // compaction of the non-zeros (any order: the 64-bit words are unique), count of the negatives
    const float *row = a.Xt + (size_t)gene * n;
    for (int i0 = 0; i0 < n; i0 += nt) {
        const int i = i0 + tid;
        const uint32_t u = i < n ? __float_as_uint(row[i]) : 0u;
        const bool nz = !zero_bits(u), ng = nz && (u >> 31);
        const unsigned long long m = __ballot(nz), mn = __ballot(ng);
        if (m) {
            uint32_t base = 0u;
            if (lane == 0) {
                base = atomicAdd(&s_cnt[0], (uint32_t)__popcll(m));
                if (mn) atomicAdd(&s_cnt[1], (uint32_t)__popcll(mn));
            }
            base = __shfl(base, 0);
            const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (nz && at < (uint32_t)P) S[at] = ((unsigned long long)order_key(u) << 32) | (uint32_t)i;
        }
    }
    for (int p = nnz + tid; p < P; p += nt) S[p] = ~0ull;                                // (sorts last: no finite key is ~0)
    __syncthreads();

    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += nt) {
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const unsigned long long x = S[lo], y = S[hi];
                if ((x > y) == ((lo & k) == 0)) {
                    S[lo] = y;
                    S[hi] = x;
                }
            }
            __syncthreads();
        }

    // doubled midrank of every sorted position; tie term of the non-zero runs
    const uint32_t neg = s_cnt[1], zeros = (uint32_t)(n - nnz);
    long long tie = 0;
    for (int p = tid; p < nnz; p += nt) {
        const uint32_t key = (uint32_t)(S[p] >> 32);
        int lo = p, hi = p + 1;
        if (p > 0 && (uint32_t)(S[p - 1] >> 32) == key) {                                // first position with this key, in [0, p - 1]
            int l = 0, r = p - 1;
            while (l < r) {
                const int m = (l + r) >> 1;
                if ((uint32_t)(S[m] >> 32) < key) l = m + 1;
                else r = m;
            }
            lo = l;
        }
        if (p + 1 < nnz && (uint32_t)(S[p + 1] >> 32) == key) {                          // first position past this key, in [p + 2, nnz]
            int l = p + 2, r = nnz;
            while (l < r) {
                const int m = (l + r) >> 1;
                if ((uint32_t)(S[m] >> 32) <= key) l = m + 1;
                else r = m;
            }
            hi = l;
        }
        const bool isneg = key < 0x80000000u;
        mid[p] = ((uint32_t)(lo + 1 + hi) + (isneg ? 0u : 2u * zeros)) | (isneg ? 0x80000000u : 0u);
        if (lo == p) {
            const long long t = hi - lo;
            tie += t * t * t - t;
        }
    }
    for (int off = 32; off > 0; off >>= 1) tie += __shfl_xor(tie, off);
    if (lane == 0 && tie) atomicAdd(s_tie, (unsigned long long)tie);
    __syncthreads();
    if (tid == 0 && a.tie) {
        const long long z = zeros;
        a.tie[gene] = (long long)*s_tie + z * z * z - z;
    }

    const long long zmid2 = 2ll * neg + zeros + 1;
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

__global__ void __launch_bounds__(1024) k_markers_rank(MarkersArgs a)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ unsigned long long s_tie;
    __shared__ uint32_t s_cnt[2];
    unsigned long long *S = reinterpret_cast<unsigned long long *>(lds);
    uint32_t *mid = reinterpret_cast<uint32_t *>(lds + (size_t)a.lds_cap * 8);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(lds + (size_t)a.lds_cap * 12);
    uint32_t *negc = reinterpret_cast<uint32_t *>(acc + kMarkersChunk * a.K);
    for (int gene = blockIdx.x; gene < a.g; gene += gridDim.x) {
        const int nnz = a.nnz[gene];
        if (nnz <= a.lds_cap) rank_gene(a, gene, nnz, S, mid, acc, negc, &s_tie, s_cnt);
        else rank_gene(a, gene, nnz, a.slab + blockIdx.x * a.slab_stride, a.slab_mid + blockIdx.x * a.slab_stride, acc, negc, &s_tie, s_cnt);
    }
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

int next_pow2(int v)
{
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

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
    if (B < 1) return fail(MI_EINVAL, "B must be >= 1 (got %d)", B);
    if (K < 1 || K > 64) return fail(MI_EINVAL, "K must be in [1, 64] (got %d)", K);
    if (flags & ~(uint32_t)(MI_MARKERS_SUM_PLAIN | MI_MARKERS_GLOBAL)) return fail(MI_EINVAL, "unknown flags 0x%x", flags);
    if (n > MI_MARKERS_MAX_CELLS) return fail(MI_EUNSUPPORTED, "%d cells exceed %d", n, MI_MARKERS_MAX_CELLS);
    if ((double)B * (double)g * (double)K > (double)MI_MARKERS_MAX_ENTRIES)
        return fail(MI_EUNSUPPORTED, "%d labellings x %d genes x %d clusters exceed %lld output entries", B, g, K,
                    (long long)MI_MARKERS_MAX_ENTRIES);
    const size_t entries = (size_t)B * g * K;
    const int Bp = (B + kMarkersChunk - 1) / kMarkersChunk * kMarkersChunk;
    const bool force_global = (flags & MI_MARKERS_GLOBAL) != 0, want_sum = out_sum != nullptr;

    float *d_X = nullptr, *d_Xt = nullptr;
    uint16_t *d_Lt = nullptr;
    int32_t *d_sizes = nullptr, *d_nnz = nullptr, *d_npos = nullptr;
    long long *d_rank2 = nullptr, *d_tie = nullptr;
    double *d_sum = nullptr;
    unsigned long long *d_slab = nullptr;
    uint32_t *d_slab_mid = nullptr;
    return guarded([&]() -> int {
        DevBufs bufs;
        // host scans: the labels (range, cluster sizes, cell-major copy) and X (finite; non-zero cells per gene)
        std::vector<int32_t> sizes((size_t)B * K, 0), nnz((size_t)g, 0);
        std::vector<uint16_t> Lt((size_t)n * Bp, 0);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < n; ++i) {
                const uint16_t c = L[(size_t)b * n + i];
                if (c >= K) return fail(MI_EINVAL, "label %d of labelling %d, cell %d is not below K = %d", (int)c, b, i, K);
                ++sizes[(size_t)b * K + c];
                Lt[(size_t)i * Bp + b] = c;
            }
        const uint32_t *U = reinterpret_cast<const uint32_t *>(X);
        for (int i = 0; i < n; ++i) {
            const uint32_t *row = U + (size_t)i * g;
            for (int j = 0; j < g; ++j) {
                const uint32_t u = row[j];
                if ((u & 0x7f800000u) == 0x7f800000u) return fail(MI_EINVAL, "X[%d, %d] is not finite", i, j);
                nnz[j] += (u & 0x7fffffffu) != 0u;
            }
        }
        // the launch's plan: the LDS arrays hold the largest non-zero count at or below the cap, the slabs the largest above
        const int cap = force_global ? 0 : MI_MARKERS_LDS_MAX_NONZEROS;
        int max_lds = 0, max_glob = 0;
        for (int j = 0; j < g; ++j) {
            if (nnz[j] <= cap) max_lds = nnz[j] > max_lds ? nnz[j] : max_lds;
            else max_glob = nnz[j] > max_glob ? nnz[j] : max_glob;
        }
        const int lds_cap = max_lds > 0 ? next_pow2(max_lds > 16 ? max_lds : 16) : 0;          // (>= 16: keeps the arrays behind it aligned)
        const size_t slab_stride = max_glob > 0 ? (size_t)next_pow2(max_glob) : 0;
        const size_t lds_bytes = ((size_t)lds_cap * 12 + (size_t)kMarkersChunk * K * 12 + 15) & ~(size_t)15;
        const int threads = (lds_cap > 2048 || slab_stride > 2048) ? 1024 : 256;

        MI_TRY(pick_device(device));
        int cus = 0;
        HIP_TRY(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device));
        size_t grid = (size_t)(cus > 0 ? cus : 1) * 8;
        if (slab_stride && grid > kSlabBudget / (slab_stride * 12)) grid = kSlabBudget / (slab_stride * 12);
        if (grid > (size_t)g) grid = (size_t)g;
        if (grid < 1) grid = 1;

        const size_t cells = (size_t)n * g;
        HIP_TRY(bufs.alloc(&d_X, cells));
        HIP_TRY(bufs.alloc(&d_Xt, cells));
        HIP_TRY(bufs.alloc(&d_Lt, Lt.size()));
        HIP_TRY(bufs.alloc(&d_sizes, sizes.size()));
        HIP_TRY(bufs.alloc(&d_nnz, nnz.size()));
        HIP_TRY(bufs.alloc(&d_rank2, entries));
        HIP_TRY(bufs.alloc(&d_npos, entries));
        HIP_TRY(bufs.alloc(&d_tie, (size_t)g));
        if (want_sum) HIP_TRY(bufs.alloc(&d_sum, entries));
        if (slab_stride) {
            HIP_TRY(bufs.alloc(&d_slab, grid * slab_stride));
            HIP_TRY(bufs.alloc(&d_slab_mid, grid * slab_stride));
        }
        HIP_TRY(hipMemcpy(d_X, X, cells * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_Lt, Lt.data(), Lt.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_sizes, sizes.data(), sizes.size() * sizeof(int32_t), hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(d_nnz, nnz.data(), nnz.size() * sizeof(int32_t), hipMemcpyHostToDevice));

        MarkersArgs a;
        a.Xt = d_Xt; a.Lt = d_Lt; a.sizes = d_sizes; a.nnz = d_nnz;
        a.n = n; a.g = g; a.B = B; a.Bp = Bp; a.K = K; a.lds_cap = lds_cap;
        a.slab = d_slab; a.slab_mid = d_slab_mid; a.slab_stride = slab_stride;
        a.rank2 = d_rank2; a.npos = d_npos; a.tie = d_tie;
        if (lds_bytes > 64 * 1024)
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k_markers_rank), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_bytes));
        Timer tm;
        MI_TRY(tm.start(0));
        hipLaunchKernelGGL(k_markers_transpose, dim3((unsigned)((g + kMarkersTile - 1) / kMarkersTile), (unsigned)((n + kMarkersTile - 1) / kMarkersTile)),
                           dim3(256), 0, 0, d_X, d_Xt, n, g);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_markers_rank, dim3((unsigned)grid), dim3((unsigned)threads), lds_bytes, 0, a);
        HIP_TRY(hipGetLastError());
        if (want_sum) {
            // a wavefront holds 64 / B genes: with few labellings neighbouring genes coalesce in X, with many it reads Xt's row
            const bool rows = B >= kMarkersChunk;
            const size_t work = (size_t)g * B;
            hipLaunchKernelGGL(k_markers_sums, dim3((unsigned)((work + kSumThreads - 1) / kSumThreads)), dim3(kSumThreads),
                               (size_t)K * kSumThreads * sizeof(double), 0, rows ? d_Xt : d_X, rows ? (size_t)1 : (size_t)g,
                               rows ? (size_t)n : (size_t)1, d_Lt, n, g, B, Bp, K, (flags & MI_MARKERS_SUM_PLAIN) ? 1 : 0, d_sum);
            HIP_TRY(hipGetLastError());
        }
        MI_TRY(tm.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy(out_rank2, d_rank2, entries * sizeof(long long), hipMemcpyDeviceToHost));
        if (out_npos) HIP_TRY(hipMemcpy(out_npos, d_npos, entries * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (out_sum) HIP_TRY(hipMemcpy(out_sum, d_sum, entries * sizeof(double), hipMemcpyDeviceToHost));
        if (out_tie) HIP_TRY(hipMemcpy(out_tie, d_tie, (size_t)g * sizeof(long long), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}
