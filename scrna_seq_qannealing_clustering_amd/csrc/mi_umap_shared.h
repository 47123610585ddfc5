// mi_umap_shared.h -- what chain U (umap_kernels.hip) and chain Q (mapping_kernels.hip) both use, written once: the cosine
// metric's host step and the arithmetic of one layout term.  DESIGN.md section 5d.
#pragma once

#include <cmath>
#include <vector>

#include "mi_sa_device.h"

namespace mi_sa_impl {

// the rows the cosine metric searches: every row divided by its norm (fp64 sum of squares in coordinate order, sqrt, fp64
// quotient rounded to f32; an all-zero row stays zero).  May throw std::bad_alloc (run under guarded()).
inline void unit_rows(const float *X, int n, int dim, std::vector<float> &unit)
{
    unit.resize((size_t)n * dim);
    for (int i = 0; i < n; ++i) {
        double ss = 0.0;
        for (int c = 0; c < dim; ++c) ss += (double)X[(size_t)i * dim + c] * (double)X[(size_t)i * dim + c];
        const double nrm = std::sqrt(ss);
        for (int c = 0; c < dim; ++c)
            unit[(size_t)i * dim + c] = nrm > 0.0 ? (float)((double)X[(size_t)i * dim + c] / nrm) : 0.0f;
    }
}

// mapping_kernels.hip: chain Q1 on DEVICE pointers, for mi_umap_query_knn_f32 and anchor_kernels.hip.  d_nn: m x k indices into
// R by ascending (d2, index), 1 <= k <= min(n, 64), nothing excluded; d_dist (nullable): the metric's m x k f32 distances
// (MI_UMAP_EUCLIDEAN: sqrt of the search's d2).  The caller has checked the points (mi_snn_check_points on both sets together).
int mi_query_knn_dev(const float *dR, int n, const float *dQ, int m, int dim, int k, int metric, int32_t *d_nn, float *d_dist);

template <int C>
__device__ __forceinline__ void load_y(const float *__restrict__ Y, int v, float (&y)[C])
{
    if constexpr (C == 2) {
        const f32x2 t = *reinterpret_cast<const f32x2 *>(Y + (size_t)v * 2);
        y[0] = t.x; y[1] = t.y;
    } else {
#pragma unroll
        for (int c = 0; c < C; ++c) y[c] = Y[(size_t)v * C + c];
    }
}

__device__ __forceinline__ float clamp4(float x) { return fminf(fmaxf(x, -4.0f), 4.0f); }

// s^b for s > 0 on v_log_f32 / v_exp_f32 with reduced arguments: log2 s = e + log2 m with m in [1/2, 1) (the instruction's error
// stays one f32 step of a number below 1), the product with b in fp64, and 2^x = 2^rint(x) * v_exp_f32(x - rint(x)).  About one
// f32 step of error in all, where exp2(b * log2(s)) on the raw arguments loses |b log2 s| of them.
__device__ __forceinline__ double log2_split(float s)
{
    return (double)__builtin_amdgcn_frexp_expf(s) + (double)__builtin_amdgcn_logf(__builtin_amdgcn_frexp_mantf(s));
}

__device__ __forceinline__ float exp2_split(double x)
{
    const double xi = rint(x);
    return ldexpf(__builtin_amdgcn_exp2f((float)(x - xi)), (int)xi);
}

}  // namespace mi_sa_impl
