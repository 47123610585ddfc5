// coassoc_kernels.hip -- co-association (consensus) statistics of a set of labellings on the i8 matrix cores (gfx950).
// C ABI: include/mi_metrics.h (mi_coassociation_u16) and mi_sa_problem_coassociation (include/mi_sa.h, mi_sa.hip).
//
// C_g[i, j] = #{reads r of group g : L[r, i] == L[r, j]} = (onehot(L_g)^T onehot(L_g))[i, j]: a product of 0/1 matrices
// with the CELLS as the outer dimensions and (read, label) as the inner one, exact on v_mfma_i32_16x16x64_i8 (i32
// accumulation, an entry is at most Rg).  The n x n product is never stored unless the caller asks for it: every tile is
// reduced in its epilogue into the histogram of its entries and the per-cell sums per reference cluster.
//
//   k_coassoc_prep   uint16 labels -> one byte per (read, cell), rows of npad bytes (npad a multiple of 128), hole seats,
//                    cells past n and reads past Rg: 0xFF, a byte that matches no label
//   k_coassoc_mfma   M2.  One workgroup of 4 wavefronts per tile of 128 x 128 cells on or above the diagonal of the block
//                    grid (a persistent loop over the tiles of its group, numbered row by row: mi_tri_tiles.h turns the
//                    number into the tile, the text agreement_kernels.hip uses and a host program checks); wavefront (wi, wj) owns 64 x 64 cells = 4 x 4
//                    accumulators of 16 x 16.  The two operand panels (128 cells x 128 reads, bytes, cells contiguous per
//                    read) are staged in LDS once per workgroup and read chunk; every wavefront builds its own one-hot
//                    fragments from them (no SIMD mate can do vector work beside an MFMA stream).
//   k_coassoc_hist   sums the per-workgroup histograms (int64)
//   k_coassoc_edges  M3.  edge[g][e] = C_g[eu[e], ev[e]] straight from the label bytes for any n: a block of edges per
//                    workgroup, the group's labels staged through LDS in read chunks while a chunk of >= 4 reads fits.
//
// Operand maps of v_mfma_i32_16x16x64_i8 (agreement_kernels.hip pins them): lane l holds A[row l & 15][the 16 k of lane
// group l >> 4] and B[the same 16 k][col l & 15], 16 bytes each; register q of the accumulator is C[row 4 (l >> 4) + q]
// [col l & 15].  The inner dimension of one MFMA is 64 (read, label) slots: labels are padded to Kp = 16 KB (KB = 1, 2, 4)
// and a k-step holds 4 / KB reads; lane group gq holds read gq / KB, labels 16 (gq % KB) .. + 15, so a lane's fragment is
// the one-hot of ONE label byte over 16 labels: byte x = label - 16 (gq % KB) set when x < 16 (dword x >> 2, byte x & 3),
// nothing set for any other label and for 0xFF.  A and B use the same construction on their own cell, so the two
// operands agree on the slot order by construction.  Accumulator (ta, tb) of a wavefront covers cells 4 m + ta (rows,
// m = MFMA row) and 4 m' + tb (columns): the four label bytes a lane needs per operand and k-step are one aligned dword.
//
// Histogram: per-workgroup LDS bins (uint32, Rg + 1 of them), LDS atomics, written once per workgroup to its own row of
// a partial table and summed by k_coassoc_hist; no atomics to global memory.  Row sums: per tile LDS [128][64] int32 for
// the row cells and for the column cells (they alias the dead operand panels), then one 64-bit atomic add per non-zero
// (cell, cluster) to the output.  All integer: the result does not depend on the order.
#include <vector>

#include "../../include/mi_metrics.h"
#include "mi_sa_device.h"
#include "mi_tri_tiles.h"

namespace mi_sa_impl {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kTile = 128;                 // cells per tile side
constexpr int kChunk = 128;                // reads per LDS chunk
constexpr int kPanelStride = 192;          // bytes per read row of a panel: 48 dwords, so the four lane groups of a ds_read_b32 hit disjoint banks
constexpr int kPanelBytes = kChunk * kPanelStride;               // 24 KB
constexpr int kScratchBytes = 2 * kTile * 64 * 4;                // 64 KB: row-sum scratch, aliases the two panels (48 KB)
constexpr unsigned kNoLabel = 0xFFu;
constexpr int kEdgeBlock = 1024;           // edges per workgroup pass of M3
constexpr int kEdgeLds = 64 * 1024;

// labels of group row r (row stride ld, columns [0, cols)) -> bytes; rows [Rg, Rp) and columns [cols, npad) are padding
__global__ void __launch_bounds__(256) k_coassoc_prep(const uint16_t *__restrict__ L, size_t ld, int cols, int Rg, int Rp,
                                                      const uint32_t *__restrict__ meta, int npad, uint8_t *__restrict__ lab8)
{
    const int row = blockIdx.x;                                  // g * Rp + r
    const int g = row / Rp, r = row - g * Rp;
    const uint16_t *src = L + ((size_t)g * Rg + (r < Rg ? r : 0)) * ld;
    uint8_t *out = lab8 + (size_t)row * npad;
    for (int i = threadIdx.x; i < npad; i += 256) {
        unsigned v = kNoLabel;
        if (r < Rg && i < cols && !(meta && (meta[i] >> 31))) {
            const unsigned l = src[i];
            if (l < 64u) v = l;                                  // (labels are validated < K <= 64 by the callers)
        }
        out[i] = (uint8_t)v;
    }
}

struct CoDev {
    const uint8_t *lab8;                   // [G][Rp][npad]
    const uint8_t *ref8;                   // [G][npad] reference labels (0xFF: hole / padding), or nullptr
    const uint32_t *meta;                  // nullable: bit 31 = hole seat
    int npad, n, Rg, Rp, nb, Kref;
    long long tpg;                         // tiles per group = nb (nb + 1) / 2
    unsigned long long *part;              // [G][gridDim.x][Rg + 1] per-workgroup histograms, or nullptr
    unsigned long long *rowsum;            // [G][n][Kref], or nullptr
    int *counts;                           // [G][n][n], or nullptr
};

template <int KB>
__device__ __forceinline__ i32x4 onehot16(unsigned w, int t, unsigned base)
{
    const unsigned x = ((w >> (8 * t)) & 0xFFu) - base;          // >= 16 (wraps) for every label outside this lane group's 16
    const unsigned q = x >> 2, s = 1u << ((x & 3u) << 3);
    return i32x4{(int)(q == 0u ? s : 0u), (int)(q == 1u ? s : 0u), (int)(q == 2u ? s : 0u), (int)(q == 3u ? s : 0u)};
}

template <int KB>
__global__ void __launch_bounds__(256) k_coassoc_mfma(CoDev g)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    uint8_t *panA = reinterpret_cast<uint8_t *>(lds), *panB = panA + kPanelBytes;
    int *rsI = reinterpret_cast<int *>(lds), *rsJ = rsI + kTile * 64;                // after the main loop only
    unsigned *bins = reinterpret_cast<unsigned *>(lds + kScratchBytes);              // [Rg + 1]
    constexpr int RPS = 4 / KB;                                                      // reads per k-step
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wi = wave >> 1, wj = wave & 1, gq = lane >> 4, m16 = lane & 15;
    const int grp = blockIdx.y;
    const unsigned base = 16u * (unsigned)(gq % KB);
    const int rsub = gq / KB;                                                        // this lane group's read inside a k-step
    const uint8_t *labg = g.lab8 + (size_t)grp * g.Rp * g.npad;
    const uint8_t *refg = g.ref8 ? g.ref8 + (size_t)grp * g.npad : nullptr;
    if (g.part)
        for (int v = tid; v <= g.Rg; v += 256) bins[v] = 0u;
    for (long long q = blockIdx.x; q < g.tpg; q += gridDim.x) {
        int bi, bj;
        mi_tri::tile_of(q, g.nb, &bi, &bj);                      // tile q -> (bi, bj), bi <= bj (mi_tri_tiles.h)
        const bool diag = bi == bj;
        const int I0 = bi * kTile, J0 = bj * kTile;
        i32x4 acc[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) acc[a][b] = i32x4{0, 0, 0, 0};
        for (int r0 = 0; r0 < g.Rp; r0 += kChunk) {
            const int rows = g.Rp - r0 < kChunk ? g.Rp - r0 : kChunk;                // a multiple of 4
            __syncthreads();                                                         // the previous chunk (or epilogue) is done with the LDS
            for (int x = tid; x < rows * 8; x += 256) {                              // 8 x 16 bytes per read row and panel
                const int rr = x >> 3, c16 = (x & 7) * 16;
                const uint8_t *src = labg + (size_t)(r0 + rr) * g.npad;
                *reinterpret_cast<uint4 *>(panA + rr * kPanelStride + c16) = *reinterpret_cast<const uint4 *>(src + I0 + c16);
                *reinterpret_cast<uint4 *>(panB + rr * kPanelStride + c16) = *reinterpret_cast<const uint4 *>(src + J0 + c16);
            }
            __syncthreads();
            const uint8_t *pa = panA + rsub * kPanelStride + wi * 64 + 4 * m16;
            const uint8_t *pb = panB + rsub * kPanelStride + wj * 64 + 4 * m16;
            const int steps = rows / RPS;
            for (int s = 0; s < steps; ++s) {
                const unsigned wa = *reinterpret_cast<const unsigned *>(pa + s * RPS * kPanelStride);
                const unsigned wb = *reinterpret_cast<const unsigned *>(pb + s * RPS * kPanelStride);
                i32x4 fa[4], fb[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    fa[t] = onehot16<KB>(wa, t, base);
                    fb[t] = onehot16<KB>(wb, t, base);
                }
#pragma unroll
                for (int a = 0; a < 4; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        acc[a][b] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[a], fb[b], acc[a][b], 0, 0, 0);
            }
        }
        // epilogue.  acc[a][b][qq] = C[i][j], i = I0 + 64 wi + 4 (4 gq + qq) + a, j = J0 + 64 wj + 4 m16 + b
        const int ib = I0 + 64 * wi + 16 * gq, jb = J0 + 64 * wj + 4 * m16;
        unsigned okI = 0u, okJ = 0u;                                                  // cell is inside [0, n) and no hole
        unsigned char refI[16], refJ[4];
#pragma unroll
        for (int x = 0; x < 16; ++x) {                                                // x = 4 qq + a
            const int i = ib + x;
            const bool ok = i < g.n && !(g.meta && (g.meta[i] >> 31));
            okI |= ok ? 1u << x : 0u;
            refI[x] = refg ? refg[i] : (unsigned char)0;
        }
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int j = jb + b;
            const bool ok = j < g.n && !(g.meta && (g.meta[j] >> 31));
            okJ |= ok ? 1u << b : 0u;
            refJ[b] = refg ? refg[j] : (unsigned char)0;
        }
        if (g.part) {
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int x = 4 * qq + a;
                        if (((okI >> x) & 1u) && ((okJ >> b) & 1u) && ib + x < jb + b) atomicAdd(&bins[acc[a][b][qq]], 1u);
                    }
        }
        if (g.counts) {
            int *cg = g.counts + (size_t)grp * g.n * g.n;
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int i = ib + 4 * qq + a, j = jb + b;
                        if (i < g.n && j < g.n) {
                            cg[(size_t)i * g.n + j] = acc[a][b][qq];
                            if (!diag) cg[(size_t)j * g.n + i] = acc[a][b][qq];      // a diagonal tile holds both halves itself
                        }
                    }
        }
        if (g.rowsum) {
            __syncthreads();                                                         // every wavefront is done with the panels
            for (int x = tid; x < 2 * kTile * 64; x += 256) rsI[x] = 0;
            __syncthreads();
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b)
#pragma unroll
                    for (int qq = 0; qq < 4; ++qq) {
                        const int x = 4 * qq + a;
                        const int v = acc[a][b][qq];
                        if (((okI >> x) & 1u) && ((okJ >> b) & 1u) && ib + x != jb + b && v != 0) {
                            atomicAdd(&rsI[(ib + x - I0) * 64 + refJ[b]], v);
                            if (!diag) atomicAdd(&rsJ[(jb + b - J0) * 64 + refI[x]], v);
                        }
                    }
            __syncthreads();
            unsigned long long *rg = g.rowsum + (size_t)grp * g.n * g.Kref;
            for (int x = tid; x < kTile * g.Kref; x += 256) {
                const int cell = x / g.Kref, c = x - cell * g.Kref;
                const int vi = rsI[cell * 64 + c];
                if (vi && I0 + cell < g.n) atomicAdd(&rg[(size_t)(I0 + cell) * g.Kref + c], (unsigned long long)vi);
                if (!diag) {
                    const int vj = rsJ[cell * 64 + c];
                    if (vj && J0 + cell < g.n) atomicAdd(&rg[(size_t)(J0 + cell) * g.Kref + c], (unsigned long long)vj);
                }
            }
        }
    }
    if (g.part) {
        __syncthreads();
        unsigned long long *out = g.part + ((size_t)grp * gridDim.x + blockIdx.x) * ((size_t)g.Rg + 1);
        for (int v = tid; v <= g.Rg; v += 256) out[v] = bins[v];
    }
}

__global__ void __launch_bounds__(256) k_coassoc_hist(const unsigned long long *__restrict__ part, int wgs, int Rg,
                                                      long long *__restrict__ hist)
{
    const int v = blockIdx.x * 256 + threadIdx.x, grp = blockIdx.y;
    if (v > Rg) return;
    const unsigned long long *p = part + (size_t)grp * wgs * ((size_t)Rg + 1) + v;
    unsigned long long s = 0;
    for (int w = 0; w < wgs; ++w) s += p[(size_t)w * ((size_t)Rg + 1)];
    hist[(size_t)grp * ((size_t)Rg + 1) + v] = (long long)s;
}

// chunk = reads per LDS chunk (0: read the label bytes from global memory, n too wide for a useful chunk)
__global__ void __launch_bounds__(256) k_coassoc_edges(const uint8_t *__restrict__ lab8, int npad, int Rg, int Rp, int chunk,
                                                       const int *__restrict__ eu, const int *__restrict__ ev, long long m,
                                                       int *__restrict__ edge)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const uint8_t *labg = lab8 + (size_t)blockIdx.y * Rp * npad;
    int *out = edge + (size_t)blockIdx.y * m;
    const int tid = threadIdx.x;
    for (long long e0 = (long long)blockIdx.x * kEdgeBlock; e0 < m; e0 += (long long)gridDim.x * kEdgeBlock) {
        int u[4], w[4], cnt[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long e = e0 + tid + 256 * k;
            u[k] = e < m ? eu[e] : 0;
            w[k] = e < m ? ev[e] : 0;
            cnt[k] = 0;
        }
        if (chunk > 0) {
            for (int r0 = 0; r0 < Rg; r0 += chunk) {
                const int rows = Rg - r0 < chunk ? Rg - r0 : chunk;
                __syncthreads();
                const uint4 *src = reinterpret_cast<const uint4 *>(labg + (size_t)r0 * npad);
                for (int x = tid; x < rows * (npad / 16); x += 256) reinterpret_cast<uint4 *>(lds)[x] = src[x];
                __syncthreads();
                for (int r = 0; r < rows; ++r) {
                    const uint8_t *row = reinterpret_cast<const uint8_t *>(lds) + (size_t)r * npad;
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const unsigned a = row[u[k]], b = row[w[k]];
                        cnt[k] += (a == b && a != kNoLabel) ? 1 : 0;
                    }
                }
            }
        } else {
            for (int r = 0; r < Rg; ++r) {
                const uint8_t *row = labg + (size_t)r * npad;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const unsigned a = row[u[k]], b = row[w[k]];
                    cnt[k] += (a == b && a != kNoLabel) ? 1 : 0;
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const long long e = e0 + tid + 256 * k;
            if (e < m) out[e] = cnt[k];
        }
    }
}

template <int KB>
int launch_coassoc(const CoDev &g, int wgs, int G, size_t lds, hipStream_t st)
{
    MI_TRY(allow_lds(k_coassoc_mfma<KB>, lds));
    hipLaunchKernelGGL((k_coassoc_mfma<KB>), dim3((unsigned)wgs, (unsigned)G), dim3(256), lds, st, g);
    return MI_OK;
}

}  // namespace

int mi_coassociation_dev(const CoassocArgs &in, hipStream_t st, int64_t *out_hist, int64_t *out_rowsum, int32_t *out_edge,
                         int32_t *out_counts, float *out_kernel_ms)
{
    const int G = in.groups, Rg = in.R / G, Rp = (Rg + 3) / 4 * 4, n = in.cols;
    const int npad = (n + kTile - 1) / kTile * kTile, nb = npad / kTile;
    const bool m2 = out_hist || out_rowsum || out_counts, m3 = out_edge != nullptr && in.m > 0;
    if (out_kernel_ms) *out_kernel_ms = 0.0f;
    if (Rg > MI_COASSOC_MAX_READS)
        return fail(MI_EUNSUPPORTED, "%d reads per group exceed MI_COASSOC_MAX_READS = %d", Rg, MI_COASSOC_MAX_READS);
    if (out_counts && (double)G * n * n > (double)MI_COASSOC_MAX_COUNT_ENTRIES)
        return fail(MI_EUNSUPPORTED, "%d co-association matrices of %d x %d exceed %d entries", G, n, n, MI_COASSOC_MAX_COUNT_ENTRIES);
    if (out_rowsum && !in.ref) return fail(MI_EINVAL, "out_rowsum needs a reference labelling");
    if (!m2 && !m3) return MI_OK;
    const int KB = in.K <= 16 ? 1 : (in.K <= 32 ? 2 : 4);
    const long long tpg = (long long)nb * (nb + 1) / 2;
    uint8_t *d_lab = nullptr, *d_ref = nullptr;
    unsigned long long *d_part = nullptr, *d_rowsum = nullptr;
    long long *d_hist = nullptr;
    int *d_counts = nullptr, *d_eu = nullptr, *d_ev = nullptr, *d_edge = nullptr;
    return guarded([&]() -> int {
        DevBufs bufs;
        int dev = 0, cus = 256;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        if (cus < 1) cus = 256;
        // workgroups per group: one per CU over all groups, never so few that a workgroup's uint32 bins could wrap
        long long want = (cus + G - 1) / G;
        const long long floor_wgs = (tpg + 131071) / 131072;                         // 131072 tiles x 16384 pairs = 2^31
        if (want < floor_wgs) want = floor_wgs;
        const int wgs = (int)(want < tpg ? want : tpg);
        HIP_TRY(bufs.alloc(&d_lab, (size_t)G * Rp * npad));
        if (m2) {
            if (out_hist) {
                HIP_TRY(bufs.alloc(&d_part, (size_t)G * wgs * ((size_t)Rg + 1)));
                HIP_TRY(bufs.alloc(&d_hist, (size_t)G * ((size_t)Rg + 1)));
            }
            if (out_rowsum) {
                std::vector<uint8_t> ref8((size_t)G * npad, (uint8_t)kNoLabel);
                for (int g = 0; g < G; ++g)
                    for (int i = 0; i < n; ++i) ref8[(size_t)g * npad + i] = (uint8_t)in.ref[(size_t)g * n + i];
                HIP_TRY(bufs.alloc(&d_ref, ref8.size()));
                HIP_TRY(hipMemcpyAsync(d_ref, ref8.data(), ref8.size(), hipMemcpyHostToDevice, st));
                HIP_TRY(hipStreamSynchronize(st));                                   // (ref8 is a host temporary)
                HIP_TRY(bufs.alloc(&d_rowsum, (size_t)G * n * in.Kref));
                HIP_TRY(hipMemsetAsync(d_rowsum, 0, (size_t)G * n * in.Kref * sizeof(unsigned long long), st));
            }
            if (out_counts) HIP_TRY(bufs.alloc(&d_counts, (size_t)G * n * n));
        }
        if (m3) {
            HIP_TRY(bufs.alloc(&d_eu, (size_t)in.m));
            HIP_TRY(bufs.alloc(&d_ev, (size_t)in.m));
            HIP_TRY(bufs.alloc(&d_edge, (size_t)G * in.m));
            HIP_TRY(hipMemcpyAsync(d_eu, in.eu, (size_t)in.m * sizeof(int), hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(d_ev, in.ev, (size_t)in.m * sizeof(int), hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
        }
        Timer tm;
        MI_TRY(tm.start(st));
        hipLaunchKernelGGL(k_coassoc_prep, dim3((unsigned)(G * Rp)), dim3(256), 0, st, in.L, in.ld, n, Rg, Rp, in.meta, npad, d_lab);
        HIP_TRY(hipGetLastError());
        if (m2) {
            CoDev g;
            g.lab8 = d_lab; g.ref8 = out_rowsum ? d_ref : nullptr; g.meta = in.meta;
            g.npad = npad; g.n = n; g.Rg = Rg; g.Rp = Rp; g.nb = nb; g.Kref = in.Kref; g.tpg = tpg;
            g.part = d_part; g.rowsum = d_rowsum; g.counts = d_counts;
            const size_t lds = (size_t)kScratchBytes + ((size_t)Rg + 1) * sizeof(unsigned);
            int rl;
            if (KB == 1) rl = launch_coassoc<1>(g, wgs, G, lds, st);
            else if (KB == 2) rl = launch_coassoc<2>(g, wgs, G, lds, st);
            else rl = launch_coassoc<4>(g, wgs, G, lds, st);
            if (rl) return rl;
            HIP_TRY(hipGetLastError());
            if (out_hist) {
                hipLaunchKernelGGL(k_coassoc_hist, dim3((unsigned)((Rg + 1 + 255) / 256), (unsigned)G), dim3(256), 0, st,
                                   (const unsigned long long *)d_part, wgs, Rg, d_hist);
                HIP_TRY(hipGetLastError());
            }
        }
        if (m3) {
            int chunk = kEdgeLds / npad;
            chunk = chunk >= 4 ? (chunk < Rg ? chunk : Rg) : 0;
            const long long eblocks = (in.m + kEdgeBlock - 1) / kEdgeBlock;
            const long long cap = (long long)(4 * cus + G - 1) / G;
            const int ewgs = (int)(eblocks < cap ? eblocks : cap);
            hipLaunchKernelGGL(k_coassoc_edges, dim3((unsigned)ewgs, (unsigned)G), dim3(256), (size_t)chunk * npad, st,
                               (const uint8_t *)d_lab, npad, Rg, Rp, chunk, (const int *)d_eu, (const int *)d_ev, (long long)in.m, d_edge);
            HIP_TRY(hipGetLastError());
        }
        MI_TRY(tm.stop(st, out_kernel_ms));
        if (out_hist) HIP_TRY(hipMemcpy(out_hist, d_hist, (size_t)G * ((size_t)Rg + 1) * sizeof(long long), hipMemcpyDeviceToHost));
        if (out_rowsum) HIP_TRY(hipMemcpy(out_rowsum, d_rowsum, (size_t)G * n * in.Kref * sizeof(long long), hipMemcpyDeviceToHost));
        if (out_counts) HIP_TRY(hipMemcpy(out_counts, d_counts, (size_t)G * n * n * sizeof(int), hipMemcpyDeviceToHost));
        if (m3) HIP_TRY(hipMemcpy(out_edge, d_edge, (size_t)G * in.m * sizeof(int), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

// shapes, labels and edges that both entry points check the same way (everything here is host data)
int mi_coassociation_check(int R, int n, int K, int groups, const uint16_t *ref, int Kref, const int32_t *eu, const int32_t *ev,
                           int64_t m, const int64_t *out_rowsum, const int32_t *out_edge)
{
    if (n < 1) return fail(MI_EINVAL, "n must be >= 1 (got %d)", n);
    if (R < 1) return fail(MI_EINVAL, "R must be >= 1 (got %d)", R);
    if (K < 1 || K > 64) return fail(MI_EINVAL, "K must be in [1, 64] (got %d)", K);
    if (groups < 1 || R % groups != 0) return fail(MI_EINVAL, "R = %d is not a multiple of groups = %d", R, groups);
    if (out_rowsum && !ref) return fail(MI_EINVAL, "out_rowsum needs a reference labelling");
    if (ref) {
        if (Kref < 1 || Kref > 64) return fail(MI_EINVAL, "Kref must be in [1, 64] (got %d)", Kref);
        for (size_t e = 0; e < (size_t)groups * n; ++e)
            if (ref[e] >= Kref) return fail(MI_EINVAL, "label %d of ref[%zu][%zu] outside [0, %d)", ref[e], e / n, e % n, Kref);
    }
    if (m < 0 || m > 0x7fffffffll) return fail(MI_EINVAL, "m must be in [0, 2^31) (got %lld)", (long long)m);
    if (out_edge && m > 0) {
        if (!eu || !ev) return fail(MI_EINVAL, "out_edge needs eu and ev");
        for (int64_t e = 0; e < m; ++e)
            if (eu[e] < 0 || eu[e] >= n || ev[e] < 0 || ev[e] >= n)
                return fail(MI_EINVAL, "edge %lld = (%d, %d) outside [0, %d)", (long long)e, eu[e], ev[e], n);
    }
    return MI_OK;
}

}  // namespace mi_sa_impl
using namespace mi_sa_impl;

extern "C" int mi_coassociation_u16(const uint16_t *L, int R, int n, int K, int groups, const uint16_t *ref, int Kref,
                                    const int32_t *eu, const int32_t *ev, int64_t m, int device, int64_t *out_hist,
                                    int64_t *out_rowsum, int32_t *out_edge, int32_t *out_counts, float *out_kernel_ms)
{
    if (!L) return fail(MI_EINVAL, "L is NULL");
    if (const int rc = mi_coassociation_check(R, n, K, groups, ref, Kref, eu, ev, m, out_rowsum, out_edge)) return rc;
    for (size_t e = 0; e < (size_t)R * n; ++e)
        if (L[e] >= K) return fail(MI_EINVAL, "label %d of L[%zu][%zu] outside [0, %d)", L[e], e / n, e % n, K);
    if (R / groups > MI_COASSOC_MAX_READS)
        return fail(MI_EUNSUPPORTED, "%d reads per group exceed MI_COASSOC_MAX_READS = %d", R / groups, MI_COASSOC_MAX_READS);
    if (out_counts && (double)groups * n * n > (double)MI_COASSOC_MAX_COUNT_ENTRIES)
        return fail(MI_EUNSUPPORTED, "%d co-association matrices of %d x %d exceed %d entries", groups, n, n, MI_COASSOC_MAX_COUNT_ENTRIES);
    MI_TRY(pick_device(device));
    uint16_t *d_L = nullptr;
    return guarded([&]() -> int {
        DevBufs bufs;
        HIP_TRY(bufs.upload(&d_L, L, (size_t)R * n));
        CoassocArgs a;
        a.L = d_L; a.ld = (size_t)n; a.R = R; a.cols = n; a.K = K; a.groups = groups; a.meta = nullptr;
        a.ref = ref; a.Kref = ref ? Kref : 1; a.eu = eu; a.ev = ev; a.m = out_edge ? m : 0;
        return mi_coassociation_dev(a, 0, out_hist, out_rowsum, out_edge, out_counts, out_kernel_ms);
    });
}
