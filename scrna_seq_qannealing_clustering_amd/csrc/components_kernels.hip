// components_kernels.hip -- batched connected components of one shared graph under a per-item edge filter (gfx950).
// C ABI: include/mi_metrics.h (mi_graph_components) and mi_sa_problem_components (include/mi_sa.h, mi_sa.hip).
//
// One graph (CSR, or the row-major adjacency a structured problem keeps in HBM), B items.  Item b sees the stored entry
// (i, j) iff L[b, i] == L[b, j] (when labellings are given) and keep[b, e] != 0 (when a mask is given); an edge connects
// its ends when one stored direction is live; self loops connect nothing.  Per item: a component id per cell, numbered
// 0 .. C_b - 1 in ascending order of each component's smallest cell, and C_b.
//
//   k_components<LDS>   one workgroup per item.  parent[] (one uint32 per cell) lives in LDS together with the item's
//                       label row (LDS = true; 6 B per cell, 4 B without labels) or, for n beyond kComponentsLdsMaxCells,
//                       in HBM, in the item's row of the output itself (LDS = false).  The adjacency is streamed from L2,
//                       which all items share.
//
// Min-hooking with pointer jumping (Shiloach-Vishkin; the FastSV form keeps only the atomic minimum):
//   hook      every live entry (i, j) with parent[i] != parent[j]: atomicMin(parent[max], min) over the two parents;
//   compress  parent[i] = parent[parent[i]] until nothing moves (every tree becomes a star);
// repeated until a hook round changes nothing.  parent[x] <= x always and parent[x] is in x's component, so the forest
// never has a cycle and a tree's root is its smallest cell.  Hooks read stars: both parents are roots, the larger root
// hangs itself below the smaller, whichever side of the edge it is on.  A root that is a local minimum among its
// neighbour trees is hooked in the following round at the latest (its neighbour has joined a smaller root by then), so
// every tree at least doubles within two rounds: O(log n) rounds of O(log n) jumps, no iteration cap, no dependence on
// the diameter.  The loop ends when a whole round has read only stars and found every live entry inside one star, i.e.
// parent[i] = smallest cell of i's component: a function of the input alone, whatever order the atomics landed in.
//
// Final pass: roots flagged (parent[i] == i, not a hole), a block scan over the cells in chunks of the workgroup's size
// gives every root its rank, kept in place as 0x80000000 | rank; every other cell then reads its root's rank.
// Stores: ordinary vector stores and the HIP atomics only.
#include "../../include/mi_metrics.h"
#include "mi_sa_device.h"

namespace mi_sa_impl {
namespace {

constexpr uint32_t kRootFlag = 0x80000000u;

template <bool LDS>
__device__ __forceinline__ uint32_t par_load(uint32_t *par, uint32_t i)
{
    if (LDS) return __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __hip_atomic_load(par + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);       // (past the CU's vector cache: atomics land in L2)
}

template <bool LDS>
__device__ __forceinline__ void par_store(uint32_t *par, uint32_t i, uint32_t v)
{
    if (LDS) __hip_atomic_store(par + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    else __hip_atomic_store(par + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__device__ __forceinline__ uint32_t par_min(uint32_t *par, uint32_t i, uint32_t v)
{
    if (LDS) return __hip_atomic_fetch_min(par + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    return __hip_atomic_fetch_min(par + i, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool LDS>
__global__ void __launch_bounds__(1024) k_components(ComponentsArgs a, int32_t *__restrict__ out, int32_t *__restrict__ count)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    __shared__ int s_wave[16];
    const int n = a.n, tid = threadIdx.x, nt = blockDim.x, lane = tid & 63, wave = tid >> 6, nw = nt >> 6;
    const size_t b = blockIdx.x;
    int32_t *outb = out + b * (size_t)n;
    uint32_t *par = LDS ? reinterpret_cast<uint32_t *>(lds) : reinterpret_cast<uint32_t *>(outb);
    const bool has_l = a.L != nullptr;
    const uint16_t *Lg = has_l ? a.L + b * a.ldl : nullptr;
    uint16_t *Ll = reinterpret_cast<uint16_t *>(lds + (size_t)n * 4);                    // LDS form with labels only
    const uint8_t *keep = a.keep ? a.keep + b * (size_t)a.nnz : nullptr;
    auto label = [&](int i) -> unsigned { return LDS ? (unsigned)Ll[i] : (unsigned)Lg[i]; };

    for (int i = tid; i < n; i += nt) {
        par_store<LDS>(par, (uint32_t)i, (uint32_t)i);
        if (LDS && has_l) Ll[i] = Lg[i];
    }
    __syncthreads();

    for (;;) {
        int changed = 0;
        for (int i = tid; i < n; i += nt) {
            long long e0, e1;
            if (a.rows) {
                const uint32_t m = a.meta[i];
                if (m >> 31) continue;                                                   // a hole seat: no cell, no edges
                e0 = (long long)i * a.D;
                e1 = e0 + (long long)((m >> 8) & 0x7fffffu);
            } else {
                e0 = a.rowptr[i];
                e1 = a.rowptr[i + 1];
            }
            const unsigned li = has_l ? label(i) : 0u;
            uint32_t pi = par_load<LDS>(par, (uint32_t)i);
            for (long long e = e0; e < e1; ++e) {
                const int j = a.rows ? (int)a.rows[e].x : a.col[e];
                if (j == i) continue;
                if (has_l && label(j) != li) continue;
                if (keep && !keep[e]) continue;
                const uint32_t pj = par_load<LDS>(par, (uint32_t)j);
                if (pi == pj) continue;
                const uint32_t hi = pi > pj ? pi : pj, lo = pi > pj ? pj : pi;
                if (par_min<LDS>(par, hi, lo) > lo) changed = 1;
                pi = lo;                                                                 // (in i's component: what the next entry hooks with)
            }
        }
        if (!__syncthreads_or(changed)) break;
        for (;;) {
            int moved = 0;
            for (int i = tid; i < n; i += nt) {
                const uint32_t p = par_load<LDS>(par, (uint32_t)i);
                const uint32_t gp = par_load<LDS>(par, p);
                if (gp != p) {
                    par_store<LDS>(par, (uint32_t)i, gp);
                    moved = 1;
                }
            }
            if (!__syncthreads_or(moved)) break;
        }
    }

    // every tree is a star.  Roots -> 0x80000000 | rank, rank by ascending cell: a scan over chunks of nt cells
    int base = 0;
    for (int c0 = 0; c0 < n; c0 += nt) {
        const int i = c0 + tid;
        bool root = false;
        if (i < n) {
            root = par_load<LDS>(par, (uint32_t)i) == (uint32_t)i;
            if (a.rows && (a.meta[i] >> 31)) root = false;
        }
        const unsigned long long m = __ballot(root);
        if (lane == 0) s_wave[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < nw; ++w) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (root) par_store<LDS>(par, (uint32_t)i, kRootFlag | (uint32_t)(base + before + __popcll(m & ((1ull << lane) - 1ull))));
        base += total;
        __syncthreads();                                                                 // (s_wave is rewritten by the next chunk)
    }
    // cells below a root take its rank (a root's entry is not touched here, a non-root's entry is read by nobody else)
    for (int i = tid; i < n; i += nt) {
        if (a.rows && (a.meta[i] >> 31)) {
            if (LDS) outb[i] = -1;                                                       // (global form: after the barrier below)
            continue;
        }
        const uint32_t p = par_load<LDS>(par, (uint32_t)i);
        if (p & kRootFlag) {
            if (LDS) outb[i] = (int32_t)(p & ~kRootFlag);
            continue;
        }
        const int32_t id = (int32_t)(par_load<LDS>(par, p) & ~kRootFlag);
        if (LDS) outb[i] = id;
        else par_store<LDS>(par, (uint32_t)i, (uint32_t)id);
    }
    if (!LDS) {
        __syncthreads();
        for (int i = tid; i < n; i += nt) {                                              // the roots and the holes, in place
            if (a.rows && (a.meta[i] >> 31)) {
                outb[i] = -1;
                continue;
            }
            const uint32_t p = par_load<LDS>(par, (uint32_t)i);
            if (p & kRootFlag) par_store<LDS>(par, (uint32_t)i, p & ~kRootFlag);
        }
    }
    if (tid == 0) count[b] = base;
}

}  // namespace

int mi_components_dev(const ComponentsArgs &a, int B, bool force_global, hipStream_t st, int32_t *out_labels,
                      int32_t *out_count, float *out_kernel_ms)
{
    const int n = a.n;
    if (out_kernel_ms) *out_kernel_ms = 0.0f;
    if ((double)B * (double)n > (double)MI_COMPONENTS_MAX_ENTRIES)
        return fail(MI_EUNSUPPORTED, "%d items of %d cells exceed %lld output entries", B, n, (long long)MI_COMPONENTS_MAX_ENTRIES);
    const bool use_lds = !force_global && n <= MI_COMPONENTS_LDS_MAX_CELLS;
    const size_t lds = use_lds ? (((size_t)n * (a.L ? 6 : 4) + 15) & ~(size_t)15) : 0;
    // small items: more workgroups per CU beat more threads per item
    const int threads = n <= 4096 ? 256 : 1024;
    int32_t *d_out = nullptr, *d_count = nullptr;
    return guarded([&]() -> int {
        DevBufs bufs;
        HIP_TRY(bufs.alloc(&d_out, (size_t)B * n));
        HIP_TRY(bufs.alloc(&d_count, (size_t)B));
        Timer tm;
        MI_TRY(tm.start(st));
        if (use_lds) {
            MI_TRY(allow_lds(k_components<true>, lds));
            hipLaunchKernelGGL(k_components<true>, dim3((unsigned)B), dim3((unsigned)threads), lds, st, a, d_out, d_count);
        } else {
            hipLaunchKernelGGL(k_components<false>, dim3((unsigned)B), dim3((unsigned)threads), 0, st, a, d_out, d_count);
        }
        MI_TRY(tm.stop(st, out_kernel_ms));
        HIP_TRY(hipMemcpy(out_labels, d_out, (size_t)B * n * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(out_count, d_count, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

}  // namespace mi_sa_impl
using namespace mi_sa_impl;

extern "C" int mi_graph_components(const int32_t *rowptr, const int32_t *col, int n, const uint16_t *L, const uint8_t *keep,
                                   int B, int device, uint32_t flags, int32_t *out_labels, int32_t *out_count,
                                   float *out_kernel_ms)
{
    if (!rowptr || !out_labels || !out_count) return fail(MI_EINVAL, "NULL argument");
    if (n < 1) return fail(MI_EINVAL, "n must be >= 1 (got %d)", n);
    if (B < 1) return fail(MI_EINVAL, "B must be >= 1 (got %d)", B);
    if (flags & ~(uint32_t)MI_COMPONENTS_GLOBAL) return fail(MI_EINVAL, "unknown flags 0x%x", flags);
    if (rowptr[0] != 0) return fail(MI_EINVAL, "rowptr[0] must be 0 (got %d)", rowptr[0]);
    for (int i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) return fail(MI_EINVAL, "rowptr is not monotone at %d", i);
    const int64_t nnz = rowptr[n];
    if (nnz > 0 && !col) return fail(MI_EINVAL, "col is NULL");
    for (int64_t e = 0; e < nnz; ++e)
        if (col[e] < 0 || col[e] >= n) return fail(MI_EINVAL, "col[%lld] = %d outside [0, %d)", (long long)e, col[e], n);
    if ((double)B * (double)n > (double)MI_COMPONENTS_MAX_ENTRIES)
        return fail(MI_EUNSUPPORTED, "%d items of %d cells exceed %lld output entries", B, n, (long long)MI_COMPONENTS_MAX_ENTRIES);
    MI_TRY(pick_device(device));
    int32_t *d_rowptr = nullptr, *d_col = nullptr;
    uint16_t *d_L = nullptr;
    uint8_t *d_keep = nullptr;
    return guarded([&]() -> int {
        DevBufs bufs;
        HIP_TRY(bufs.upload(&d_rowptr, rowptr, (size_t)n + 1));
        HIP_TRY(bufs.upload(&d_col, col, (size_t)nnz));           // (without edges: a pointer all the same, nothing copied)
        if (L) HIP_TRY(bufs.upload(&d_L, L, (size_t)B * n));
        if (keep && nnz > 0) HIP_TRY(bufs.upload(&d_keep, keep, (size_t)B * (size_t)nnz));
        ComponentsArgs a;
        a.rowptr = d_rowptr; a.col = d_col; a.n = n; a.nnz = nnz;
        a.L = d_L; a.ldl = (size_t)n; a.keep = d_keep;
        return mi_components_dev(a, B, (flags & MI_COMPONENTS_GLOBAL) != 0, 0, out_labels, out_count, out_kernel_ms);
    });
}
