// mi_markers_plan.h -- the host plan of the ranking pass of csrc/markers_kernels.hip, from an upper bound of every gene's
// non-zero count: the exact count of a dense matrix (host scan or k_markers_count), the stored count of a sparse handle
// (colptr).  No HIP, no device code: plain g++ compiles it (tests/host/markers_plan_main.cpp runs it under the sanitizers).
#pragma once

#include <cstddef>
#include <cstdint>

namespace mi_markers_plan {

struct Plan {
    int lds_cap = 0;               // entries of the LDS arrays: a power of two >= the largest count served in LDS, or 0
    size_t slab_stride = 0;        // entries of one workgroup's slab in HBM: a power of two >= the largest count above the cap, or 0
    size_t lds_bytes = 0;          // dynamic LDS of the launch: 12 B per LDS entry + 12 B per (labelling of the chunk, cluster)
    int threads = 256;             // workgroup size
    size_t grid = 1;               // workgroups (each owns one slab)
};

inline int next_pow2(int v)
{
    int p = 1;
    while (p < v) p <<= 1;
    return p;
}

// counts[j] = colptr[j + 1] - colptr[j]: the stored entries of gene j, an upper bound of its non-zeros
inline void stored_counts(const int64_t *colptr, int g, int32_t *counts)
{
    for (int j = 0; j < g; ++j) counts[j] = (int32_t)(colptr[(size_t)j + 1] - colptr[j]);
}

// cap: a gene with at most this many planned entries is ranked in LDS (0: every gene in the HBM form); chunk: labellings
// scored per pass; cus: compute units of the device; slab_budget: bytes of HBM for all slabs.  A gene with count 0 needs
// neither array.
inline Plan plan(const int32_t *counts, int g, int K, int cap, int chunk, int cus, size_t slab_budget)
{
    Plan p;
    int max_lds = 0, max_glob = 0;
    for (int j = 0; j < g; ++j) {
        if (counts[j] <= cap) max_lds = counts[j] > max_lds ? counts[j] : max_lds;
        else max_glob = counts[j] > max_glob ? counts[j] : max_glob;
    }
    p.lds_cap = max_lds > 0 ? next_pow2(max_lds > 16 ? max_lds : 16) : 0;                 // (>= 16: keeps the arrays behind it aligned)
    p.slab_stride = max_glob > 0 ? (size_t)next_pow2(max_glob) : 0;
    p.lds_bytes = ((size_t)p.lds_cap * 12 + (size_t)chunk * K * 12 + 15) & ~(size_t)15;
    p.threads = (p.lds_cap > 2048 || p.slab_stride > 2048) ? 1024 : 256;
    p.grid = (size_t)(cus > 0 ? cus : 1) * 8;
    if (p.slab_stride && p.grid > slab_budget / (p.slab_stride * 12)) p.grid = slab_budget / (p.slab_stride * 12);
    if (p.grid > (size_t)g) p.grid = (size_t)g;
    if (p.grid < 1) p.grid = 1;
    return p;
}

}  // namespace mi_markers_plan
