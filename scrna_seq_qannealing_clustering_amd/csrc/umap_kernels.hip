// umap_kernels.hip -- UMAP on MI355X (gfx950): kNN distances -> smooth kNN distances -> fuzzy union graph -> a deterministic
// SGD layout.  C ABI and the kernels' layouts: include/mi_umap.h.  Specification: DESIGN.md section 5d ("chain U"),
// restated in numpy by tests/umap_reference.py.
//
// The reference draws every result with Seurat's RunUMAP (R/pbmc3k/Pbmc3k_assess_QA_clusters.Rmd:94-108,
// R/kidney/Kidney_data.Rmd:133-155); this file replaces that call.  Nothing here accumulates with floating-point atomics and
// every random number is a Philox block addressed by (vertex, entry, epoch, sample): two runs are bit-identical.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mi_umap.h"
#include "mi_umap_shared.h"

namespace mi_sa_impl {
namespace {

// ---- U1: distances of the kNN table ----------------------------------------------------------------------------------------
// d2 = k_knn's chain: fmaf over the coordinates in ascending order (its zero padding adds fmaf(0, 0, d) = d)
__global__ void __launch_bounds__(256) k_umap_dist(const float *__restrict__ X, int n, int dim, int k, int metric,
                                                   const int32_t *__restrict__ nn, float *__restrict__ dist)
{
    const long long total = (long long)n * k;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const int i = (int)(e / k), j = nn[e];
        const float *xi = X + (size_t)i * dim, *xj = X + (size_t)j * dim;
        float d = 0.0f;
        for (int c = 0; c < dim; ++c) {
            const float df = xi[c] - xj[c];
            d = __fmaf_rn(df, df, d);
        }
        dist[e] = metric == MI_UMAP_COSINE ? d * 0.5f : __fsqrt_rn(d);
    }
}

// ---- U2: smooth kNN distances, fp64 ----------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_umap_rho(int n, int k, const float *__restrict__ dist, double *__restrict__ rho,
                                                  double *__restrict__ mean)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double r = INFINITY, s = 0.0;
    for (int p = 0; p < k; ++p) {
        const double d = (double)dist[(size_t)i * k + p];
        s += d;
        if (p >= 1 && d > 0.0 && d < r) r = d;
    }
    rho[i] = std::isinf(r) ? 0.0 : r;
    mean[i] = s / (double)k;
}

// exactly 64 steps, no early exit: the result does not depend on the last bits of exp
__global__ void __launch_bounds__(256) k_umap_sigma(int n, int k, double target, double mean_all,
                                                    const float *__restrict__ dist, const double *__restrict__ rho,
                                                    const double *__restrict__ mean, double *__restrict__ sigma)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double r = rho[i];
    const float *di = dist + (size_t)i * k;
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int step = 0; step < 64; ++step) {
        double psum = 0.0;
        for (int p = 1; p < k; ++p) {
            const double x = (double)di[p] - r;
            psum += x > 0.0 ? exp(-(x / mid)) : 1.0;
        }
        if (psum > target) {
            hi = mid;
            mid = (lo + hi) / 2.0;
        } else {
            lo = mid;
            mid = std::isinf(hi) ? 2.0 * mid : (lo + hi) / 2.0;
        }
    }
    const double floor_ = 1e-3 * (r > 0.0 ? mean[i] : mean_all);
    sigma[i] = mid > floor_ ? mid : floor_;
}

// ---- U3: fuzzy union --------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double membership(float d, double rho, double sigma)
{
    const double x = (double)d - rho;
    return x <= 0.0 ? 1.0 : exp(-(x / sigma));
}

// One wavefront per row i, one lane per candidate: slots 0 .. k-2 are the row's own neighbours nn[i, 1 + s], the others the
// points that list i (RN(i)), minus i itself and minus those already among the neighbours.  Writes the row's candidates
// (column, or -1 for a slot that holds nothing) at i (k - 1) + rn_ptr[i] and the number of survivors to deg[i].
__global__ void __launch_bounds__(256) k_umap_union_raw(int n, int k, const int32_t *__restrict__ nn,
                                                        const float *__restrict__ dist, const double *__restrict__ rho,
                                                        const double *__restrict__ sigma, const int *__restrict__ rn_ptr,
                                                        const int32_t *__restrict__ rn_idx, int32_t *__restrict__ raw_col,
                                                        float *__restrict__ raw_w, int *__restrict__ deg)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                          // (wave-uniform)
    const int r0 = rn_ptr[i], L = (k - 1) + (rn_ptr[i + 1] - r0);
    const size_t base = (size_t)i * (k - 1) + r0;
    const int32_t *ni = nn + (size_t)i * k;
    const double rho_i = rho[i], sig_i = sigma[i];
    int count = 0;
    for (int s0 = 0; s0 < L; s0 += 64) {
        const int s = s0 + lane;
        bool valid = false;
        if (s < L) {
            int j;
            double a = 0.0;
            if (s < k - 1) {
                j = ni[1 + s];
                a = membership(dist[(size_t)i * k + 1 + s], rho_i, sig_i);
                valid = true;
            } else {
                j = rn_idx[r0 + (s - (k - 1))];
                valid = j != i;
                for (int p = 1; p < k && valid; ++p) valid = ni[p] != j;
            }
            float wf = 0.0f;
            if (valid) {
                double b = 0.0;
                const int32_t *nj = nn + (size_t)j * k;
                for (int q = 1; q < k; ++q)
                    if (nj[q] == i) {
                        b = membership(dist[(size_t)j * k + q], rho[j], sigma[j]);
                        break;
                    }
                wf = (float)(a + b - a * b);                     // a + b and a * b commute: row j computes the same bits
                valid = wf > 0.0f;
            }
            raw_col[base + s] = valid ? j : -1;
            raw_w[base + s] = wf;
        }
        count += __popcll(__ballot(valid));
    }
    if (lane == 0) deg[i] = count;
}

// rank by counting: the columns of a row are distinct, so an entry's place is the number of smaller columns.  O(L^2 / 64) per
// row; the order the reverse lists were filled in does not show in the result.
__global__ void __launch_bounds__(256) k_umap_union_sort(int n, int k, const int *__restrict__ rn_ptr,
                                                         const int32_t *__restrict__ raw_col,
                                                         const float *__restrict__ raw_w, const int *__restrict__ rowptr,
                                                         int32_t *__restrict__ col, float *__restrict__ w,
                                                         unsigned int *__restrict__ stats)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int r0 = rn_ptr[i], L = (k - 1) + (rn_ptr[i + 1] - r0);
    const size_t base = (size_t)i * (k - 1) + r0;
    const int out = rowptr[i];
    unsigned int wmax = 0u;
    for (int s = lane; s < L; s += 64) {
        const int j = raw_col[base + s];
        if (j < 0) continue;
        int rank = 0;
        for (int t = 0; t < L; ++t) {
            const int jt = raw_col[base + t];
            rank += (jt >= 0 && jt < j) ? 1 : 0;
        }
        const float wf = raw_w[base + s];
        col[out + rank] = j;
        w[out + rank] = wf;
        const unsigned int bits = __float_as_uint(wf);          // positive floats order as their bits
        wmax = bits > wmax ? bits : wmax;
    }
    if (wmax) atomicMax(&stats[0], wmax);
    if (lane == 0) atomicMax(&stats[1], (unsigned int)(rowptr[i + 1] - out));
}

// ---- U4: one epoch of the layout (load_y, clamp4, log2_split, exp2_split: mi_umap_shared.h) -------------------------------------
// A group of G lanes owns vertex v = (global thread) / G; lane l of the group takes entries l, l + G, ... of the row in
// ascending order, each with its negatives, and the G partial sums meet in a butterfly.  s^b and s^(b-1): exp2_split.
template <int G, int C>
__global__ void __launch_bounds__(256) k_umap_layout(int n, const uint32_t *__restrict__ rowptr,
                                                     const int32_t *__restrict__ col, const float *__restrict__ prob,
                                                     const float *__restrict__ Yin, float *__restrict__ Yout, float a,
                                                     float b, float alpha, int t, int neg, uint32_t k0, uint32_t k1)
{
    const int gl = threadIdx.x & (G - 1);
    const int v = (int)(((long long)blockIdx.x * 256 + threadIdx.x) / G);
    if (v >= n) return;                                          // (the whole group leaves)
    const uint32_t e0 = rowptr[v], e1 = rowptr[v + 1];
    float yi[C];
    load_y<C>(Yin, v, yi);
    if (e0 == e1) {                                              // an empty row never moves
        if (gl == 0) {
#pragma unroll
            for (int c = 0; c < C; ++c) Yout[(size_t)v * C + c] = yi[c];
        }
        return;
    }
    float g[C];
#pragma unroll
    for (int c = 0; c < C; ++c) g[c] = 0.0f;
    const float tf0 = (float)t, tf1 = (float)(t + 1);
    const float m2ab = -2.0f * a * b, twob = 2.0f * b;
    const double bd = (double)b, bm1d = (double)(b - 1.0f);
    for (unsigned long long E = (unsigned long long)e0 + gl; E < e1; E += G) {
        const float pe = prob[E];
        if ((int)floorf(tf1 * pe) - (int)floorf(tf0 * pe) < 1) continue;
        {
            float yj[C], d[C], s = 0.0f;
            load_y<C>(Yin, col[E], yj);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                d[c] = yi[c] - yj[c];
                s = c == 0 ? d[c] * d[c] : s + d[c] * d[c];
            }
            if (s > 0.0f) {
                const double l = log2_split(s);
                const float coef = (m2ab * exp2_split(bm1d * l)) / (a * exp2_split(bd * l) + 1.0f);
#pragma unroll
                for (int c = 0; c < C; ++c) g[c] += clamp4(coef * d[c]);
            }
        }
        for (int q = 0; q < neg; ++q) {
            uint32_t r[4];
            philox4x32_10((uint32_t)v, (uint32_t)E, (uint32_t)t, (uint32_t)q, k0, k1, r);
            const int j = (int)(r[0] % (uint32_t)n);
            if (j == v) continue;
            float yj[C], d[C], s = 0.0f;
            load_y<C>(Yin, j, yj);
#pragma unroll
            for (int c = 0; c < C; ++c) {
                d[c] = yi[c] - yj[c];
                s = c == 0 ? d[c] * d[c] : s + d[c] * d[c];
            }
            if (s > 0.0f) {
                const float coef = twob / ((0.001f + s) * (a * exp2_split(bd * log2_split(s)) + 1.0f));
#pragma unroll
                for (int c = 0; c < C; ++c) g[c] += clamp4(coef * d[c]);
            } else {
#pragma unroll
                for (int c = 0; c < C; ++c) g[c] += 4.0f;
            }
        }
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] += __shfl_xor(g[c], off, 64);
    }
    if (gl == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) Yout[(size_t)v * C + c] = yi[c] + alpha * g[c];
    }
}

template <int G, int C>
void launch_layout(int n, const uint32_t *rowptr, const int32_t *col, const float *prob, const float *Yin, float *Yout,
                   float a, float b, float alpha, int t, int neg, uint32_t k0, uint32_t k1)
{
    const unsigned blocks = (unsigned)(((long long)n * G + 255) / 256);
    hipLaunchKernelGGL((k_umap_layout<G, C>), dim3(blocks), dim3(256), 0, 0, n, rowptr, col, prob, Yin, Yout, a, b, alpha, t,
                       neg, k0, k1);
}

}  // namespace
}  // namespace mi_sa_impl
using namespace mi_sa_impl;

struct mi_umap_graph {
    int n = 0, dim = 0, k = 0, metric = 0, device = 0, max_degree = 0;
    int stage = 1;                   // 1 = kNN, 2 = smoothed, 3 = union built
    long long nnz = 0;
    float w_max = 0.0f;
    DevArray<int32_t> d_nn, d_col;
    DevArray<float> d_dist, d_w;
    DevArray<double> d_rho, d_sigma, d_mean;
    DevArray<int> d_ptr;
};

extern "C" {

int mi_umap_destroy(mi_umap_graph *g)
{
    if (!g) return MI_OK;
    (void)hipSetDevice(g->device);
    delete g;
    return MI_OK;
}

int mi_umap_knn_f32(const float *X, int n, int dim, int k, int metric, int device, mi_umap_graph **out, float *out_kernel_ms)
{
    if (!X || !out) return fail(MI_EINVAL, "NULL argument");
    if (n < 2 || dim < 1 || dim > 64) return fail(MI_EINVAL, "need n >= 2 and 1 <= dim <= 64 (got n=%d dim=%d)", n, dim);
    if (k < 2 || k > 64 || k > n) return fail(MI_EINVAL, "need 2 <= k <= min(64, n) (got k=%d)", k);
    if (metric != MI_UMAP_EUCLIDEAN && metric != MI_UMAP_COSINE) return fail(MI_EINVAL, "unknown metric %d", metric);
    if (n > MI_UMAP_MAX_POINTS) return fail(MI_EUNSUPPORTED, "n = %d exceeds %d", n, MI_UMAP_MAX_POINTS);
    if ((long long)n * k >= (1ll << 30)) return fail(MI_EUNSUPPORTED, "n * k = %lld reaches 2^30", (long long)n * k);
    const size_t cells = (size_t)n * dim;
    // the domain of k_knn (mi_snn_check_points: finite cells, no fp32 overflow of a squared distance), on the rows the search
    // sees -- the normalised ones for the cosine metric, which always pass the range check -- and before any device work
    std::vector<float> unit;
    const float *src = X;
    const int rc0 = guarded([&]() -> int {
        for (size_t e = 0; e < cells; ++e)
            if (!std::isfinite(X[e])) return fail(MI_EINVAL, "X[%lld, %lld] is not finite", (long long)(e / dim), (long long)(e % dim));
        if (metric == MI_UMAP_COSINE) {
            unit_rows(X, n, dim, unit);
            src = unit.data();
        }
        return mi_snn_check_points(src, n, dim);
    });
    if (rc0) return rc0;
    MI_TRY(pick_device(device));
    mi_umap_graph *g = nullptr;
    const int rc = guarded([&]() -> int {
        g = new mi_umap_graph();
        g->n = n; g->dim = dim; g->k = k; g->metric = metric; g->device = device;
        DevBufs tmp;
        float *dX = nullptr;
        HIP_TRY(tmp.upload(&dX, src, cells));
        HIP_TRY(g->d_nn.resize((size_t)n * k));
        HIP_TRY(g->d_dist.resize((size_t)n * k));
        Timer tm;
        MI_TRY(tm.start(0));
        MI_TRY(mi_snn_knn_dev(dX, n, dim, k, g->d_nn, 0));
        const long long total = (long long)n * k;
        const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
        hipLaunchKernelGGL(k_umap_dist, dim3(blocks), dim3(256), 0, 0, dX, n, dim, k, metric, g->d_nn, g->d_dist);
        MI_TRY(tm.stop(0, out_kernel_ms));
        return MI_OK;
    });
    if (rc) { mi_umap_destroy(g); return rc; }
    *out = g;
    return MI_OK;
}

int mi_umap_fetch_knn(mi_umap_graph *g, int32_t *nn, float *dist)
{
    if (!g) return fail(MI_EINVAL, "NULL handle");
    HIP_TRY(hipSetDevice(g->device));
    const size_t cells = (size_t)g->n * g->k;
    if (nn) HIP_TRY(hipMemcpy(nn, g->d_nn, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (dist) HIP_TRY(hipMemcpy(dist, g->d_dist, cells * sizeof(float), hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi_umap_smooth(mi_umap_graph *g, float *out_kernel_ms)
{
    if (!g) return fail(MI_EINVAL, "NULL handle");
    HIP_TRY(hipSetDevice(g->device));
    return guarded([&]() -> int {
        const int n = g->n, k = g->k;
        HIP_TRY(g->d_rho.resize((size_t)n));
        HIP_TRY(g->d_sigma.resize((size_t)n));
        HIP_TRY(g->d_mean.resize((size_t)n));
        g->stage = 1; g->nnz = 0; g->max_degree = 0; g->w_max = 0.0f;
        const unsigned blocks = (unsigned)((n + 255) / 256);
        float ms0 = 0.0f, ms1 = 0.0f;
        {
            Timer tm;
            MI_TRY(tm.start(0));
            hipLaunchKernelGGL(k_umap_rho, dim3(blocks), dim3(256), 0, 0, n, k, g->d_dist, g->d_rho, g->d_mean);
            MI_TRY(tm.stop(0, &ms0));
        }
        std::vector<double> mean((size_t)n);
        HIP_TRY(hipMemcpy(mean.data(), g->d_mean, (size_t)n * sizeof(double), hipMemcpyDeviceToHost));
        double tot = 0.0;
        for (int i = 0; i < n; ++i) tot += mean[(size_t)i];       // index order: the fixed order of the specification
        const double mean_all = tot / (double)n;
        {
            Timer tm;
            MI_TRY(tm.start(0));
            hipLaunchKernelGGL(k_umap_sigma, dim3(blocks), dim3(256), 0, 0, n, k, std::log2((double)k), mean_all, g->d_dist,
                               g->d_rho, g->d_mean, g->d_sigma);
            MI_TRY(tm.stop(0, &ms1));
        }
        if (out_kernel_ms) *out_kernel_ms = ms0 + ms1;
        g->stage = 2;
        return MI_OK;
    });
}

int mi_umap_fetch_smooth(mi_umap_graph *g, double *rho, double *sigma)
{
    if (!g) return fail(MI_EINVAL, "NULL handle");
    if (g->stage < 2) return fail(MI_ESTATE, "mi_umap_fetch_smooth before mi_umap_smooth");
    HIP_TRY(hipSetDevice(g->device));
    if (rho) HIP_TRY(hipMemcpy(rho, g->d_rho, (size_t)g->n * sizeof(double), hipMemcpyDeviceToHost));
    if (sigma) HIP_TRY(hipMemcpy(sigma, g->d_sigma, (size_t)g->n * sizeof(double), hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi_umap_union(mi_umap_graph *g, float *out_kernel_ms)
{
    if (!g) return fail(MI_EINVAL, "NULL handle");
    if (g->stage < 2) return fail(MI_ESTATE, "mi_umap_union before mi_umap_smooth");
    HIP_TRY(hipSetDevice(g->device));
    return guarded([&]() -> int {
        const int n = g->n, k = g->k;
        g->d_ptr.reset(); g->d_col.reset(); g->d_w.reset();
        g->stage = 2; g->nnz = 0; g->max_degree = 0; g->w_max = 0.0f;
        DevBufs tmp;
        int *d_cnt = nullptr, *d_rn_ptr = nullptr, *d_cursor = nullptr, *d_deg = nullptr;
        int32_t *d_rn_idx = nullptr, *d_raw_col = nullptr;
        float *d_raw_w = nullptr;
        unsigned int *d_stats = nullptr;
        const size_t raw = (size_t)n * (k - 1) + (size_t)n * k;   // every row: its k - 1 neighbours + its reverse list
        HIP_TRY(tmp.alloc(&d_cnt, (size_t)n + 1));
        HIP_TRY(tmp.alloc(&d_rn_ptr, (size_t)n + 1));
        HIP_TRY(tmp.alloc(&d_cursor, (size_t)n + 1));
        HIP_TRY(tmp.alloc(&d_deg, (size_t)n + 1));
        HIP_TRY(tmp.alloc(&d_rn_idx, (size_t)n * k));
        HIP_TRY(tmp.alloc(&d_raw_col, raw));
        HIP_TRY(tmp.alloc(&d_raw_w, raw));
        HIP_TRY(tmp.alloc(&d_stats, 2));
        HIP_TRY(g->d_ptr.resize((size_t)n + 1));
        HIP_TRY(hipMemsetAsync(d_cnt, 0, ((size_t)n + 1) * sizeof(int), 0));
        HIP_TRY(hipMemsetAsync(d_cursor, 0, ((size_t)n + 1) * sizeof(int), 0));
        HIP_TRY(hipMemsetAsync(d_stats, 0, 2 * sizeof(unsigned int), 0));
        const unsigned rows = (unsigned)((n + 3) / 4);
        float ms0 = 0.0f, ms1 = 0.0f;
        {
            Timer tm;
            MI_TRY(tm.start(0));
            MI_TRY(mi_snn_reverse_lists_dev(g->d_nn, n, k, d_cnt, d_rn_ptr, d_cursor, d_rn_idx, 0));
            hipLaunchKernelGGL(k_umap_union_raw, dim3(rows), dim3(256), 0, 0, n, k, g->d_nn, g->d_dist, g->d_rho, g->d_sigma,
                               d_rn_ptr, d_rn_idx, d_raw_col, d_raw_w, d_deg);
            MI_TRY(mi_scan_exclusive_dev(d_deg, g->d_ptr, n, 0));
            MI_TRY(tm.stop(0, &ms0));
        }
        int nnz = 0;
        HIP_TRY(hipMemcpy(&nnz, g->d_ptr + n, sizeof(int), hipMemcpyDeviceToHost));
        HIP_TRY(g->d_col.resize((size_t)(nnz > 0 ? nnz : 0)));
        HIP_TRY(g->d_w.resize((size_t)(nnz > 0 ? nnz : 0)));
        {
            Timer tm;
            MI_TRY(tm.start(0));
            hipLaunchKernelGGL(k_umap_union_sort, dim3(rows), dim3(256), 0, 0, n, k, d_rn_ptr, d_raw_col, d_raw_w, g->d_ptr,
                               g->d_col, g->d_w, d_stats);
            MI_TRY(tm.stop(0, &ms1));
        }
        unsigned int stats[2] = {0u, 0u};
        HIP_TRY(hipMemcpy(stats, d_stats, sizeof stats, hipMemcpyDeviceToHost));
        g->nnz = nnz;
        g->max_degree = (int)stats[1];
        std::memcpy(&g->w_max, &stats[0], sizeof(float));
        if (out_kernel_ms) *out_kernel_ms = ms0 + ms1;
        g->stage = 3;
        return MI_OK;
    });
}

int mi_umap_info(const mi_umap_graph *g, int *n, int *k, int64_t *nnz, int *max_degree, float *w_max)
{
    if (!g) return fail(MI_EINVAL, "NULL handle");
    if (n) *n = g->n;
    if (k) *k = g->k;
    if (nnz) *nnz = g->nnz;
    if (max_degree) *max_degree = g->max_degree;
    if (w_max) *w_max = g->w_max;
    return MI_OK;
}

int mi_umap_fetch_graph(mi_umap_graph *g, int64_t *rowptr, int32_t *col, float *w)
{
    if (!g) return fail(MI_EINVAL, "NULL handle");
    if (g->stage < 3) return fail(MI_ESTATE, "mi_umap_fetch_graph before mi_umap_union");
    HIP_TRY(hipSetDevice(g->device));
    if (rowptr) {
        const int rc = guarded([&]() -> int {
            std::vector<int> tmp((size_t)g->n + 1);
            HIP_TRY(hipMemcpy(tmp.data(), g->d_ptr, tmp.size() * sizeof(int), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < tmp.size(); ++i) rowptr[i] = tmp[i];
            return MI_OK;
        });
        if (rc) return rc;
    }
    if (col && g->nnz) HIP_TRY(hipMemcpy(col, g->d_col, (size_t)g->nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (w && g->nnz) HIP_TRY(hipMemcpy(w, g->d_w, (size_t)g->nnz * sizeof(float), hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi_umap_layout_f32(int n, int c, const int64_t *rowptr, const int32_t *col, const float *w, const float *Y0, float a,
                       float b, float alpha0, int T, int neg, uint64_t seed, int device, float *Y_out, float *out_kernel_ms)
{
    if (!rowptr || !Y0 || !Y_out) return fail(MI_EINVAL, "NULL argument");
    if (n < 1) return fail(MI_EINVAL, "need n >= 1 (got %d)", n);
    if (c != 2 && c != 3) return fail(MI_EUNSUPPORTED, "n_components must be 2 or 3 (got %d)", c);
    if (n > MI_UMAP_MAX_POINTS) return fail(MI_EUNSUPPORTED, "n = %d exceeds %d", n, MI_UMAP_MAX_POINTS);
    if (T < 1 || T > MI_UMAP_MAX_EPOCHS) return fail(MI_EINVAL, "need 1 <= T <= %d (got %d)", MI_UMAP_MAX_EPOCHS, T);
    if (neg < 0 || neg > MI_UMAP_MAX_NEGATIVE) return fail(MI_EINVAL, "need 0 <= neg <= %d (got %d)", MI_UMAP_MAX_NEGATIVE, neg);
    if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(alpha0)) return fail(MI_EINVAL, "a, b and alpha0 must be finite");
    if (rowptr[0] != 0) return fail(MI_EINVAL, "rowptr[0] must be 0");
    for (int i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) return fail(MI_EINVAL, "rowptr decreases at row %d", i);
    const int64_t nnz = rowptr[n];
    if (nnz >= (1ll << 32)) return fail(MI_EUNSUPPORTED, "nnz = %lld reaches 2^32", (long long)nnz);
    if (nnz > 0 && (!col || !w)) return fail(MI_EINVAL, "NULL argument");
    float w_max = 0.0f;
    for (int i = 0; i < n; ++i)
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            if (col[e] < 0 || col[e] >= n) return fail(MI_EINVAL, "row %d: column %d outside [0, %d)", i, col[e], n);
            if (col[e] == i) return fail(MI_EINVAL, "row %d has a diagonal entry", i);
            if (e > rowptr[i] && col[e] <= col[e - 1]) return fail(MI_EINVAL, "row %d: columns are not strictly ascending", i);
            if (!std::isfinite(w[e]) || !(w[e] > 0.0f)) return fail(MI_EINVAL, "row %d: weight of column %d is not finite and positive", i, col[e]);
            w_max = w[e] > w_max ? w[e] : w_max;
        }
    const size_t cells = (size_t)n * c;
    for (size_t e = 0; e < cells; ++e)
        if (!std::isfinite(Y0[e])) return fail(MI_EINVAL, "Y0[%lld, %lld] is not finite", (long long)(e / c), (long long)(e % c));
    MI_TRY(pick_device(device));
    return guarded([&]() -> int {
        std::vector<uint32_t> ptr32((size_t)n + 1);
        for (size_t i = 0; i < ptr32.size(); ++i) ptr32[i] = (uint32_t)rowptr[i];
        std::vector<float> prob((size_t)nnz);
        for (int64_t e = 0; e < nnz; ++e) prob[(size_t)e] = w[e] / w_max;      // one f32 division
        DevBufs tmp;
        uint32_t *d_ptr = nullptr;
        int32_t *d_col = nullptr;
        float *d_prob = nullptr, *d_Y[2] = {nullptr, nullptr};
        HIP_TRY(tmp.upload(&d_ptr, ptr32.data(), ptr32.size()));
        HIP_TRY(tmp.upload(&d_col, col, (size_t)nnz));
        HIP_TRY(tmp.upload(&d_prob, prob.data(), (size_t)nnz));
        HIP_TRY(tmp.upload(&d_Y[0], Y0, cells));
        HIP_TRY(tmp.alloc(&d_Y[1], cells));
        // lanes per vertex: the smallest of 16, 32, 64 that holds the mean row length (a function of the graph alone)
        const double mean_deg = (double)nnz / (double)n;
        const int G = mean_deg > 32.0 ? 64 : (mean_deg > 16.0 ? 32 : 16);
        const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        Timer tm;
        MI_TRY(tm.start(0));
        for (int t = 0; t < T; ++t) {
            const float alpha = (float)((double)alpha0 * (1.0 - (double)t / (double)T));
            const float *in = d_Y[t & 1];
            float *outp = d_Y[(t + 1) & 1];
#define MI_UMAP_LAUNCH(GG, CC) launch_layout<GG, CC>(n, d_ptr, d_col, d_prob, in, outp, a, b, alpha, t, neg, k0, k1)
            if (c == 2) {
                if (G == 64) MI_UMAP_LAUNCH(64, 2); else if (G == 32) MI_UMAP_LAUNCH(32, 2); else MI_UMAP_LAUNCH(16, 2);
            } else {
                if (G == 64) MI_UMAP_LAUNCH(64, 3); else if (G == 32) MI_UMAP_LAUNCH(32, 3); else MI_UMAP_LAUNCH(16, 3);
            }
#undef MI_UMAP_LAUNCH
        }
        MI_TRY(tm.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy(Y_out, d_Y[T & 1], cells * sizeof(float), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

}  // extern "C"
