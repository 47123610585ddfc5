// mapping_kernels.hip -- mapping new points onto a fixed reference on MI355X (gfx950): exact kNN of a query set against another
// set -> smooth kNN distances (umap-learn's transform rule, rho = 0) -> a weighted neighbour vote (label transfer), the
// weighted-mean start and the out-of-sample UMAP layout.  C ABI: include/mi_umap.h.  Specification: DESIGN.md section 5d
// ("chain Q"), restated in numpy by tests/mapping_reference.py.
//
// The reference clusters a sub-sample and leaves every other cell at label 0
// (R/pbmc3k/Pbmc3k_data_subsampling_clusters.Rmd:34-44), and places query cells in a fitted embedding with Seurat's MapQuery
// (Pbmc3k_assess_QA_clusters.Rmd:210-237); this file is both steps.  A query depends on the reference alone, never on the other
// queries of its call: every row normalisation is the row's own, and the Philox counter carries the query's global index.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mi_umap.h"
#include "mi_umap_shared.h"

namespace mi_sa_impl {
namespace {

constexpr int kCrossThreads = 64;     // one wavefront per workgroup, as k_knn

// ---- Q1: k_knn (snn_kernels.hip) with the queries and the streamed set apart -------------------------------------------------
// One query per thread, the reference streamed through an LDS tile every lane reads at the same address, four fmaf chains in
// flight, the running top-KM list in registers.  Nothing is excluded and there is no self slot: KM >= k.
template <int DP, int KM>
__global__ void __launch_bounds__(kCrossThreads) k_knn_cross(const float *__restrict__ R, int n, const float *__restrict__ Q,
                                                             int m, int dim, int k, int32_t *__restrict__ nn)
{
    __shared__ __attribute__((aligned(16))) float tile[kCrossThreads * DP];
    const int i = blockIdx.x * kCrossThreads + threadIdx.x;
    float xq[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) xq[c] = (i < m && c < dim) ? Q[(size_t)i * dim + c] : 0.0f;
    float bd[KM];
    int bj[KM];
#pragma unroll
    for (int p = 0; p < KM; ++p) { bd[p] = INFINITY; bj[p] = INT_MAX; }

    for (int j0 = 0; j0 < n; j0 += kCrossThreads) {
        __syncthreads();
        {
            const int j = j0 + (int)threadIdx.x;
#pragma unroll
            for (int c = 0; c < DP; ++c)
                tile[threadIdx.x * DP + c] = (j < n && c < dim) ? R[(size_t)j * dim + c] : 0.0f;
        }
        __syncthreads();
        const int lim = n - j0 < kCrossThreads ? n - j0 : kCrossThreads;
        for (int jj = 0; jj < lim; jj += 4) {                     // (rows past `lim` are zero-filled and masked out by j < n)
            float d4[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const f32x4 *tp = reinterpret_cast<const f32x4 *>(tile + (jj + u) * DP);
                float d = 0.0f;
#pragma unroll
                for (int c4 = 0; c4 < DP / 4; ++c4) {
                    const f32x4 v = tp[c4];                       // same address in every lane: LDS broadcast
                    float df;
                    df = xq[4 * c4 + 0] - v.x; d = __fmaf_rn(df, df, d);
                    df = xq[4 * c4 + 1] - v.y; d = __fmaf_rn(df, df, d);
                    df = xq[4 * c4 + 2] - v.z; d = __fmaf_rn(df, df, d);
                    df = xq[4 * c4 + 3] - v.w; d = __fmaf_rn(df, df, d);
                }
                d4[u] = d;
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int j = j0 + jj + u;
                const float d = d4[u];
                if (j < n && d < bd[KM - 1]) {                    // candidates arrive by ascending j: equal d never displaces
                    bd[KM - 1] = d;
                    bj[KM - 1] = j;
#pragma unroll
                    for (int p = KM - 1; p > 0; --p) {
                        if (bd[p] < bd[p - 1]) {
                            const float td = bd[p]; bd[p] = bd[p - 1]; bd[p - 1] = td;
                            const int tj = bj[p]; bj[p] = bj[p - 1]; bj[p - 1] = tj;
                        }
                    }
                }
            }
        }
    }
    if (i < m) {
#pragma unroll
        for (int p = 0; p < KM; ++p)
            if (p < k) nn[(size_t)i * k + p] = bj[p];
    }
}

template <int DP>
void launch_knn_cross(const float *dR, int n, const float *dQ, int m, int dim, int k, int32_t *d_nn)
{
    const dim3 grid((unsigned)((m + kCrossThreads - 1) / kCrossThreads)), block(kCrossThreads);
    if (k <= 8) hipLaunchKernelGGL((k_knn_cross<DP, 8>), grid, block, 0, 0, dR, n, dQ, m, dim, k, d_nn);
    else if (k <= 16) hipLaunchKernelGGL((k_knn_cross<DP, 16>), grid, block, 0, 0, dR, n, dQ, m, dim, k, d_nn);
    else if (k <= 32) hipLaunchKernelGGL((k_knn_cross<DP, 32>), grid, block, 0, 0, dR, n, dQ, m, dim, k, d_nn);
    else hipLaunchKernelGGL((k_knn_cross<DP, 64>), grid, block, 0, 0, dR, n, dQ, m, dim, k, d_nn);
}

// d2 = the search's chain (its zero padding adds fmaf(0, 0, d) = d), then the metric's distance, as k_umap_dist
__global__ void __launch_bounds__(256) k_query_dist(const float *__restrict__ R, const float *__restrict__ Q, int m, int dim,
                                                    int k, int metric, const int32_t *__restrict__ nn,
                                                    float *__restrict__ dist)
{
    const long long total = (long long)m * k;
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < total; e += (long long)gridDim.x * 256) {
        const float *xi = Q + (size_t)(e / k) * dim, *xj = R + (size_t)nn[e] * dim;
        float d = 0.0f;
        for (int c = 0; c < dim; ++c) {
            const float df = xi[c] - xj[c];
            d = __fmaf_rn(df, df, d);
        }
        dist[e] = metric == MI_UMAP_COSINE ? d * 0.5f : __fsqrt_rn(d);
    }
}

// ---- Q2: sigma by U2's bisection with rho = 0 over all k columns, then the weights ----------------------------------------------
__global__ void __launch_bounds__(256) k_query_smooth(int m, int k, double target, const float *__restrict__ dist,
                                                      double *__restrict__ sigma, float *__restrict__ w)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const float *di = dist + (size_t)i * k;
    double s = 0.0;
    for (int p = 0; p < k; ++p) s += (double)di[p];
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int step = 0; step < 64; ++step) {                      // exactly 64 steps, no early exit
        double psum = 0.0;
        for (int p = 0; p < k; ++p) {
            const double x = (double)di[p];
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
    const double floor_ = 1e-3 * (s / (double)k);                // the row's own mean: no other query enters
    const double sg = mid > floor_ ? mid : floor_;
    sigma[i] = sg;
    for (int p = 0; p < k; ++p) {
        const double x = (double)di[p];
        w[(size_t)i * k + p] = (float)(x > 0.0 ? exp(-(x / sg)) : 1.0);
    }
}

// ---- Q3: the weighted mean of the neighbours' positions, fp64 in column order ---------------------------------------------------
template <int C>
__global__ void __launch_bounds__(256) k_query_init(int m, int k, const int32_t *__restrict__ nn, const float *__restrict__ w,
                                                    const float *__restrict__ Yref, float *__restrict__ Y0)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double num[C], den = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) num[c] = 0.0;
    for (int p = 0; p < k; ++p) {
        const double v = (double)w[(size_t)i * k + p];
        const float *y = Yref + (size_t)nn[(size_t)i * k + p] * C;
#pragma unroll
        for (int c = 0; c < C; ++c) num[c] += v * (double)y[c];
        den += v;
    }
#pragma unroll
    for (int c = 0; c < C; ++c) Y0[(size_t)i * C + c] = (float)(num[c] / den);
}

// ---- Q5: the vote.  Only a label among the row's k neighbours can win: k <= 64 candidates, no L-sized array -----------------
__global__ void __launch_bounds__(256) k_query_vote(int m, int k, int L, const int32_t *__restrict__ nn,
                                                    const float *__restrict__ w, const int32_t *__restrict__ labels,
                                                    int32_t *__restrict__ label, double *__restrict__ score,
                                                    double *__restrict__ scores)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    const int32_t *ni = nn + (size_t)i * k;
    const float *wi = w ? w + (size_t)i * k : nullptr;           // (null: the uniform vote)
    double total = 0.0;
    for (int p = 0; p < k; ++p)
        if (labels[ni[p]] >= 0) total += wi ? (double)wi[p] : 1.0;
    int best = -1;
    double best_score = 0.0;
    if (total > 0.0) {
        for (int p = 0; p < k; ++p) {
            const int l = labels[ni[p]];
            if (l < 0) continue;
            bool seen = false;
            for (int q = 0; q < p && !seen; ++q) seen = labels[ni[q]] == l;
            if (seen) continue;
            double sum = 0.0;
            for (int q = p; q < k; ++q)                          // column order; the columns before p do not hold l
                if (labels[ni[q]] == l) sum += wi ? (double)wi[q] : 1.0;
            const double sc = sum / total;
            if (scores) scores[(size_t)i * L + l] = sc;
            if (best < 0 || sc > best_score || (sc == best_score && l < best)) { best = l; best_score = sc; }
        }
    }
    label[i] = best;
    score[i] = best_score;
}

// ---- Q4: every epoch of a query in one launch -----------------------------------------------------------------------------------
// A group of G lanes owns query v; lane l holds entry l (its neighbour, its firing ratio) and every lane of the group the
// query's position, all in registers from the first epoch to the last.  Only the queries move and they never read each other:
// no second buffer, no launch per epoch; Yref comes through L2.  One term is k_umap_layout's, operation for operation.
template <int G, int C>
__global__ void __launch_bounds__(256) k_umap_transform(int m, int k, int n, const int32_t *__restrict__ nn,
                                                        const float *__restrict__ prob, const float *__restrict__ Yref,
                                                        const float *__restrict__ Y0, const float *__restrict__ alpha,
                                                        float *__restrict__ Yout, float a, float b, int T, int neg,
                                                        uint32_t q0, uint32_t k0, uint32_t k1)
{
    const int gl = threadIdx.x & (G - 1);
    const int v = (int)(((long long)blockIdx.x * 256 + threadIdx.x) / G);
    if (v >= m) return;                                          // (the whole group leaves)
    const bool live = gl < k;
    const int col = live ? nn[(size_t)v * k + gl] : 0;
    const float pe = live ? prob[(size_t)v * k + gl] : 0.0f;     // (a ratio of 0 never fires)
    float yi[C];
    load_y<C>(Y0, v, yi);
    const float m2ab = -2.0f * a * b, twob = 2.0f * b;
    const double bd = (double)b, bm1d = (double)(b - 1.0f);
    for (int t = 0; t < T; ++t) {
        float g[C];
#pragma unroll
        for (int c = 0; c < C; ++c) g[c] = 0.0f;
        if ((int)floorf((float)(t + 1) * pe) - (int)floorf((float)t * pe) >= 1) {
            {
                float yj[C], d[C], s = 0.0f;
                load_y<C>(Yref, col, yj);
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
                philox4x32_10(q0 + (uint32_t)v, (uint32_t)gl, (uint32_t)t, (uint32_t)q, k0, k1, r);
                const int j = (int)(r[0] % (uint32_t)n);         // a reference point: no index of it is the query's own
                float yj[C], d[C], s = 0.0f;
                load_y<C>(Yref, j, yj);
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
        for (int off = G / 2; off > 0; off >>= 1) {              // a + b == b + a: every lane of the group holds the same sum
#pragma unroll
            for (int c = 0; c < C; ++c) g[c] += __shfl_xor(g[c], off, 64);
        }
        const float al = alpha[t];
#pragma unroll
        for (int c = 0; c < C; ++c) yi[c] = yi[c] + al * g[c];
    }
    if (gl == 0) {
#pragma unroll
        for (int c = 0; c < C; ++c) Yout[(size_t)v * C + c] = yi[c];
    }
}

template <int G, int C>
void launch_transform(int m, int k, int n, const int32_t *nn, const float *prob, const float *Yref, const float *Y0,
                      const float *alpha, float *Yout, float a, float b, int T, int neg, uint32_t q0, uint32_t k0, uint32_t k1)
{
    const unsigned blocks = (unsigned)(((long long)m * G + 255) / 256);
    hipLaunchKernelGGL((k_umap_transform<G, C>), dim3(blocks), dim3(256), 0, 0, m, k, n, nn, prob, Yref, Y0, alpha, Yout, a, b, T,
                       neg, q0, k0, k1);
}

int check_finite(const float *X, size_t rows, int cols, const char *what)
{
    for (size_t e = 0; e < rows * (size_t)cols; ++e)
        if (!std::isfinite(X[e])) return fail(MI_EINVAL, "%s[%lld, %lld] is not finite", what, (long long)(e / cols), (long long)(e % cols));
    return MI_OK;
}

}  // namespace

// Q1 on DEVICE pointers (declared in mi_umap_shared.h): mi_umap_query_knn_f32 and chain A (anchor_kernels.hip) both come here
int mi_query_knn_dev(const float *dR, int n, const float *dQ, int m, int dim, int k, int metric, int32_t *d_nn, float *d_dist)
{
    if (dim <= 16) launch_knn_cross<16>(dR, n, dQ, m, dim, k, d_nn);
    else if (dim <= 32) launch_knn_cross<32>(dR, n, dQ, m, dim, k, d_nn);
    else launch_knn_cross<64>(dR, n, dQ, m, dim, k, d_nn);
    if (d_dist) {
        const long long total = (long long)m * k;
        const int blocks = (int)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
        hipLaunchKernelGGL(k_query_dist, dim3(blocks), dim3(256), 0, 0, dR, dQ, m, dim, k, metric, d_nn, d_dist);
    }
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // namespace mi_sa_impl
using namespace mi_sa_impl;

struct mi_umap_query {
    int n = 0, m = 0, dim = 0, k = 0, metric = 0, device = 0;
    int stage = 1;                   // 1 = kNN, 2 = smoothed
    DevArray<int32_t> d_nn;
    DevArray<float> d_dist, d_w;
    DevArray<double> d_sigma;
};

extern "C" {

int mi_umap_query_destroy(mi_umap_query *q)
{
    if (!q) return MI_OK;
    (void)hipSetDevice(q->device);
    delete q;
    return MI_OK;
}

int mi_umap_query_knn_f32(const float *R, int n, const float *Q, int m, int dim, int k, int metric, int device,
                          mi_umap_query **out, float *out_kernel_ms)
{
    if (!R || !Q || !out) return fail(MI_EINVAL, "NULL argument");
    if (n < 2 || m < 1 || dim < 1 || dim > 64)
        return fail(MI_EINVAL, "need n >= 2, m >= 1 and 1 <= dim <= 64 (got n=%d m=%d dim=%d)", n, m, dim);
    if (k < 2 || k > 64 || k > n) return fail(MI_EINVAL, "need 2 <= k <= min(64, n) (got k=%d)", k);
    if (metric != MI_UMAP_EUCLIDEAN && metric != MI_UMAP_COSINE) return fail(MI_EINVAL, "unknown metric %d", metric);
    if (n > MI_UMAP_MAX_POINTS || m > MI_UMAP_MAX_POINTS)
        return fail(MI_EUNSUPPORTED, "n = %d or m = %d exceeds %d", n, m, MI_UMAP_MAX_POINTS);
    if ((long long)m * k >= (1ll << 30)) return fail(MI_EUNSUPPORTED, "m * k = %lld reaches 2^30", (long long)m * k);
    const size_t rcells = (size_t)n * dim, qcells = (size_t)m * dim;
    // k_knn's domain on the rows the search sees, with the coordinate ranges taken over both sets: one array, R then Q
    std::vector<float> both;
    const int rc0 = guarded([&]() -> int {
        MI_TRY(check_finite(R, (size_t)n, dim, "R"));
        MI_TRY(check_finite(Q, (size_t)m, dim, "Q"));
        if (metric == MI_UMAP_COSINE) {
            std::vector<float> ur, uq;
            unit_rows(R, n, dim, ur);
            unit_rows(Q, m, dim, uq);
            both = std::move(ur);
            both.insert(both.end(), uq.begin(), uq.end());
        } else {
            both.assign(R, R + rcells);
            both.insert(both.end(), Q, Q + qcells);
        }
        return mi_snn_check_points(both.data(), n + m, dim);
    });
    if (rc0) return rc0;
    MI_TRY(pick_device(device));
    mi_umap_query *q = nullptr;
    const int rc = guarded([&]() -> int {
        q = new mi_umap_query();
        q->n = n; q->m = m; q->dim = dim; q->k = k; q->metric = metric; q->device = device;
        DevBufs tmp;
        float *dX = nullptr;
        HIP_TRY(tmp.upload(&dX, both.data(), rcells + qcells));
        const float *dR = dX, *dQ = dX + rcells;
        HIP_TRY(q->d_nn.resize((size_t)m * k));
        HIP_TRY(q->d_dist.resize((size_t)m * k));
        Timer tm;
        MI_TRY(tm.start(0));
        MI_TRY(mi_query_knn_dev(dR, n, dQ, m, dim, k, metric, q->d_nn, q->d_dist));
        MI_TRY(tm.stop(0, out_kernel_ms));
        return MI_OK;
    });
    if (rc) { mi_umap_query_destroy(q); return rc; }
    *out = q;
    return MI_OK;
}

int mi_umap_query_fetch_knn(mi_umap_query *q, int32_t *nn, float *dist)
{
    if (!q) return fail(MI_EINVAL, "NULL handle");
    HIP_TRY(hipSetDevice(q->device));
    const size_t cells = (size_t)q->m * q->k;
    if (nn) HIP_TRY(hipMemcpy(nn, q->d_nn, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (dist) HIP_TRY(hipMemcpy(dist, q->d_dist, cells * sizeof(float), hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi_umap_query_smooth(mi_umap_query *q, float *out_kernel_ms)
{
    if (!q) return fail(MI_EINVAL, "NULL handle");
    HIP_TRY(hipSetDevice(q->device));
    return guarded([&]() -> int {
        const int m = q->m, k = q->k;
        q->stage = 1;
        HIP_TRY(q->d_sigma.resize((size_t)m));
        HIP_TRY(q->d_w.resize((size_t)m * k));
        Timer tm;
        MI_TRY(tm.start(0));
        hipLaunchKernelGGL(k_query_smooth, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, m, k, std::log2((double)k),
                           q->d_dist, q->d_sigma, q->d_w);
        MI_TRY(tm.stop(0, out_kernel_ms));
        q->stage = 2;
        return MI_OK;
    });
}

int mi_umap_query_fetch_smooth(mi_umap_query *q, double *sigma, float *w)
{
    if (!q) return fail(MI_EINVAL, "NULL handle");
    if (q->stage < 2) return fail(MI_ESTATE, "mi_umap_query_fetch_smooth before mi_umap_query_smooth");
    HIP_TRY(hipSetDevice(q->device));
    if (sigma) HIP_TRY(hipMemcpy(sigma, q->d_sigma, (size_t)q->m * sizeof(double), hipMemcpyDeviceToHost));
    if (w) HIP_TRY(hipMemcpy(w, q->d_w, (size_t)q->m * q->k * sizeof(float), hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi_umap_query_vote(mi_umap_query *q, const int32_t *labels, int L, int weighted, int32_t *label, double *score,
                       double *scores, float *out_kernel_ms)
{
    if (!q) return fail(MI_EINVAL, "NULL handle");
    if (!labels || !label || !score) return fail(MI_EINVAL, "NULL argument");
    if (L < 1) return fail(MI_EINVAL, "need L >= 1 (got %d)", L);
    if (weighted != 0 && weighted != 1) return fail(MI_EINVAL, "weighted must be 0 (uniform) or 1 (fuzzy) (got %d)", weighted);
    if (weighted && q->stage < 2) return fail(MI_ESTATE, "a fuzzy mi_umap_query_vote before mi_umap_query_smooth");
    if (scores && (long long)q->m * L >= (1ll << 31))
        return fail(MI_EUNSUPPORTED, "m * L = %lld reaches 2^31", (long long)q->m * L);
    for (int j = 0; j < q->n; ++j)
        if (labels[j] < -1 || labels[j] >= L) return fail(MI_EINVAL, "labels[%d] = %d is neither -1 nor in [0, %d)", j, labels[j], L);
    HIP_TRY(hipSetDevice(q->device));
    return guarded([&]() -> int {
        const int m = q->m;
        const size_t dense = scores ? (size_t)m * L : 0;
        DevBufs tmp;
        int32_t *d_labels = nullptr, *d_label = nullptr;
        double *d_score = nullptr, *d_scores = nullptr;
        HIP_TRY(tmp.upload(&d_labels, labels, (size_t)q->n));
        HIP_TRY(tmp.alloc(&d_label, (size_t)m));
        HIP_TRY(tmp.alloc(&d_score, (size_t)m));
        if (scores) {
            HIP_TRY(tmp.alloc(&d_scores, dense));
            HIP_TRY(hipMemsetAsync(d_scores, 0, dense * sizeof(double), 0));
        }
        Timer tm;
        MI_TRY(tm.start(0));
        hipLaunchKernelGGL(k_query_vote, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, m, q->k, L, q->d_nn,
                           weighted ? (const float *)q->d_w : (const float *)nullptr, d_labels, d_label, d_score, d_scores);
        MI_TRY(tm.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy(label, d_label, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(score, d_score, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
        if (scores) HIP_TRY(hipMemcpy(scores, d_scores, dense * sizeof(double), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_umap_query_init(mi_umap_query *q, int c, const float *Yref, float *Y0, float *out_kernel_ms)
{
    if (!q) return fail(MI_EINVAL, "NULL handle");
    if (!Yref || !Y0) return fail(MI_EINVAL, "NULL argument");
    if (c != 2 && c != 3) return fail(MI_EUNSUPPORTED, "n_components must be 2 or 3 (got %d)", c);
    if (q->stage < 2) return fail(MI_ESTATE, "mi_umap_query_init before mi_umap_query_smooth");
    MI_TRY(check_finite(Yref, (size_t)q->n, c, "Yref"));
    HIP_TRY(hipSetDevice(q->device));
    return guarded([&]() -> int {
        const int m = q->m;
        DevBufs tmp;
        float *d_Yref = nullptr, *d_Y0 = nullptr;
        HIP_TRY(tmp.upload(&d_Yref, Yref, (size_t)q->n * c));
        HIP_TRY(tmp.alloc(&d_Y0, (size_t)m * c));
        const dim3 grid((unsigned)((m + 255) / 256)), block(256);
        Timer tm;
        MI_TRY(tm.start(0));
        if (c == 2) hipLaunchKernelGGL(k_query_init<2>, grid, block, 0, 0, m, q->k, q->d_nn, q->d_w, d_Yref, d_Y0);
        else hipLaunchKernelGGL(k_query_init<3>, grid, block, 0, 0, m, q->k, q->d_nn, q->d_w, d_Yref, d_Y0);
        MI_TRY(tm.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy(Y0, d_Y0, (size_t)m * c * sizeof(float), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_umap_transform_layout_f32(int m, int k, const int32_t *nn, const float *w, int n, int c, const float *Yref,
                                 const float *Y0, float a, float b, float alpha0, int T, int neg, uint64_t seed, int64_t q0,
                                 int device, float *Y_out, float *out_kernel_ms)
{
    if (!nn || !w || !Yref || !Y0 || !Y_out) return fail(MI_EINVAL, "NULL argument");
    if (m < 1 || n < 1) return fail(MI_EINVAL, "need m >= 1 and n >= 1 (got m=%d n=%d)", m, n);
    if (k < 1 || k > 64) return fail(MI_EINVAL, "need 1 <= k <= 64 (got %d)", k);
    if (c != 2 && c != 3) return fail(MI_EUNSUPPORTED, "n_components must be 2 or 3 (got %d)", c);
    if (n > MI_UMAP_MAX_POINTS || m > MI_UMAP_MAX_POINTS)
        return fail(MI_EUNSUPPORTED, "n = %d or m = %d exceeds %d", n, m, MI_UMAP_MAX_POINTS);
    if ((long long)m * k >= (1ll << 30)) return fail(MI_EUNSUPPORTED, "m * k = %lld reaches 2^30", (long long)m * k);
    if (T < 1 || T > MI_UMAP_MAX_EPOCHS) return fail(MI_EINVAL, "need 1 <= T <= %d (got %d)", MI_UMAP_MAX_EPOCHS, T);
    if (neg < 0 || neg > MI_UMAP_MAX_NEGATIVE) return fail(MI_EINVAL, "need 0 <= neg <= %d (got %d)", MI_UMAP_MAX_NEGATIVE, neg);
    if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(alpha0)) return fail(MI_EINVAL, "a, b and alpha0 must be finite");
    if (q0 < 0 || q0 + m > (int64_t)INT32_MAX)
        return fail(MI_EINVAL, "need q0 >= 0 and q0 + m <= 2^31 - 1 (got q0=%lld m=%d)", (long long)q0, m);
    return guarded([&]() -> int {
        std::vector<float> prob((size_t)m * k), alpha((size_t)T);
        for (int i = 0; i < m; ++i) {
            float top = 0.0f;
            for (int p = 0; p < k; ++p) {
                const size_t e = (size_t)i * k + p;
                if (nn[e] < 0 || nn[e] >= n) return fail(MI_EINVAL, "row %d: neighbour %d outside [0, %d)", i, nn[e], n);
                if (!std::isfinite(w[e]) || w[e] < 0.0f) return fail(MI_EINVAL, "row %d: weight %d is not finite and >= 0", i, p);
                top = w[e] > top ? w[e] : top;
            }
            if (!(top > 0.0f)) return fail(MI_EINVAL, "row %d: no positive weight", i);
            for (int p = 0; p < k; ++p) prob[(size_t)i * k + p] = w[(size_t)i * k + p] / top;    // one f32 division, by the ROW's maximum
        }
        MI_TRY(check_finite(Yref, (size_t)n, c, "Yref"));
        MI_TRY(check_finite(Y0, (size_t)m, c, "Y0"));
        for (int t = 0; t < T; ++t) alpha[(size_t)t] = (float)((double)alpha0 * (1.0 - (double)t / (double)T));
        MI_TRY(pick_device(device));
        DevBufs tmp;
        int32_t *d_nn = nullptr;
        float *d_prob = nullptr, *d_Yref = nullptr, *d_Y0 = nullptr, *d_alpha = nullptr, *d_out = nullptr;
        HIP_TRY(tmp.upload(&d_nn, nn, (size_t)m * k));
        HIP_TRY(tmp.upload(&d_prob, prob.data(), prob.size()));
        HIP_TRY(tmp.upload(&d_Yref, Yref, (size_t)n * c));
        HIP_TRY(tmp.upload(&d_Y0, Y0, (size_t)m * c));
        HIP_TRY(tmp.upload(&d_alpha, alpha.data(), alpha.size()));
        HIP_TRY(tmp.alloc(&d_out, (size_t)m * c));
        const int G = k > 32 ? 64 : (k > 16 ? 32 : 16);           // lanes per query: the smallest that holds the k entries
        const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        Timer tm;
        MI_TRY(tm.start(0));
#define MI_TRANSFORM_LAUNCH(GG, CC) \
    launch_transform<GG, CC>(m, k, n, d_nn, d_prob, d_Yref, d_Y0, d_alpha, d_out, a, b, T, neg, (uint32_t)q0, k0, k1)
        if (c == 2) {
            if (G == 64) MI_TRANSFORM_LAUNCH(64, 2); else if (G == 32) MI_TRANSFORM_LAUNCH(32, 2); else MI_TRANSFORM_LAUNCH(16, 2);
        } else {
            if (G == 64) MI_TRANSFORM_LAUNCH(64, 3); else if (G == 32) MI_TRANSFORM_LAUNCH(32, 3); else MI_TRANSFORM_LAUNCH(16, 3);
        }
#undef MI_TRANSFORM_LAUNCH
        MI_TRY(tm.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy(Y_out, d_out, (size_t)m * c * sizeof(float), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

}  // extern "C"
