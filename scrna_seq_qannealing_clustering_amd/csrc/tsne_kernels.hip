// tsne_kernels.hip -- t-SNE on MI355X (gfx950): exact kNN in passes of 64 -> perplexity calibration -> joint P (symmetric CSR)
// -> a layout with exact all-pairs repulsion, and the KL divergence.  C ABI and the kernels' layouts: include/mi_tsne.h.
// Specification: DESIGN.md section 5d ("chain T"), restated in numpy by tests/tsne_reference.py.
//
// The reference draws RunTSNE next to every RunUMAP of its normalisation notebook
// (R/pbmc3k/Pbmc3k_normalization_simulated_data.Rmd:236-237, 254-255, 272-273, 498); this file replaces that call.  Nothing here
// accumulates with floating-point atomics and every sum has a fixed order: two runs are bit-identical.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/mi_tsne.h"
#include "mi_umap_shared.h"

namespace mi_sa_impl {
namespace {

constexpr int kKnnThreads = 64;       // one wavefront per workgroup, as k_knn
constexpr int kPass = 64;             // neighbours one pass of k_knn_after collects: the register list of k_knn_cross
constexpr int kRepThreads = 256;      // points per workgroup of k_tsne_repulse = its LDS tile

// ---- T1: k_knn_cross (mapping_kernels.hip) with a floor -------------------------------------------------------------------------
// One query per thread, the points streamed through an LDS tile every lane reads at the same address, four fmaf chains in flight
// (k_knn's chain: coordinates in ascending order, the zero padding adds fmaf(0, 0, d) = d), the running top-64 in registers.
// Pass p writes entries 64 p .. min(64 p + 63, K - 1) of the row: a candidate counts only if (d, j) is lexicographically above
// the row's entry 64 p - 1, which the pass before wrote (pass 0: everything but the point itself).
template <int DP>
__global__ void __launch_bounds__(kKnnThreads) k_knn_after(const float *__restrict__ X, int n, int dim, int K, int pass,
                                                           int32_t *nn, float *d2)
{
    __shared__ __attribute__((aligned(16))) float tile[kKnnThreads * DP];
    const int i = blockIdx.x * kKnnThreads + threadIdx.x;
    float xq[DP];
#pragma unroll
    for (int c = 0; c < DP; ++c) xq[c] = (i < n && c < dim) ? X[(size_t)i * dim + c] : 0.0f;
    float fd = -1.0f;                                             // (every d is >= 0)
    int fj = -1;
    if (pass > 0 && i < n) {
        fd = d2[(size_t)i * K + pass * kPass - 1];
        fj = nn[(size_t)i * K + pass * kPass - 1];
    }
    float bd[kPass];
    int bj[kPass];
#pragma unroll
    for (int p = 0; p < kPass; ++p) { bd[p] = INFINITY; bj[p] = INT_MAX; }

    for (int j0 = 0; j0 < n; j0 += kKnnThreads) {
        __syncthreads();
        {
            const int j = j0 + (int)threadIdx.x;
#pragma unroll
            for (int c = 0; c < DP; ++c)
                tile[threadIdx.x * DP + c] = (j < n && c < dim) ? X[(size_t)j * dim + c] : 0.0f;
        }
        __syncthreads();
        const int lim = n - j0 < kKnnThreads ? n - j0 : kKnnThreads;
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
                const bool above = d > fd || (d == fd && j > fj);
                if (j < n && j != i && above && d < bd[kPass - 1]) {   // candidates arrive by ascending j: equal d never displaces
                    bd[kPass - 1] = d;
                    bj[kPass - 1] = j;
#pragma unroll
                    for (int p = kPass - 1; p > 0; --p) {
                        if (bd[p] < bd[p - 1]) {
                            const float td = bd[p]; bd[p] = bd[p - 1]; bd[p - 1] = td;
                            const int tj = bj[p]; bj[p] = bj[p - 1]; bj[p - 1] = tj;
                        }
                    }
                }
            }
        }
    }
    if (i < n) {
#pragma unroll
        for (int p = 0; p < kPass; ++p)
            if (pass * kPass + p < K) {
                nn[(size_t)i * K + pass * kPass + p] = bj[p];
                d2[(size_t)i * K + pass * kPass + p] = bd[p];
            }
    }
}

template <int DP>
void launch_knn_after(const float *dX, int n, int dim, int K, int32_t *d_nn, float *d_d2)
{
    const dim3 grid((unsigned)((n + kKnnThreads - 1) / kKnnThreads)), block(kKnnThreads);
    for (int pass = 0; pass * kPass < K; ++pass)
        hipLaunchKernelGGL((k_knn_after<DP>), grid, block, 0, 0, dX, n, dim, K, pass, d_nn, d_d2);
}

// ---- T2: perplexity calibration, fp64 --------------------------------------------------------------------------------------------
// exactly `steps` steps, no early exit: the trip count does not depend on the data
__global__ void __launch_bounds__(256) k_tsne_calibrate(int n, int K, double log_perp, int steps, const float *__restrict__ d2,
                                                        double *__restrict__ beta_out, double *__restrict__ cond)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float *di = d2 + (size_t)i * K;
    const double d0 = (double)di[0];
    double beta = 1.0, lo = -INFINITY, hi = INFINITY;
    for (int step = 0; step < steps; ++step) {
        double Z = 0.0, S = 0.0;
        for (int p = 0; p < K; ++p) {
            const double D = (double)di[p] - d0;
            const double pj = exp(-(beta * D));
            Z += pj;
            S += pj * D;
        }
        const double H = log(Z) + beta * S / Z;
        if (H > log_perp) {
            lo = beta;
            beta = std::isinf(hi) ? beta * 2.0 : (beta + hi) / 2.0;
        } else {
            hi = beta;
            beta = std::isinf(lo) ? beta / 2.0 : (beta + lo) / 2.0;
        }
    }
    double Z = 0.0;
    for (int p = 0; p < K; ++p) Z += exp(-(beta * ((double)di[p] - d0)));
    for (int p = 0; p < K; ++p) cond[(size_t)i * K + p] = exp(-(beta * ((double)di[p] - d0))) / Z;
    beta_out[i] = beta;
}

// ---- T3: joint P --------------------------------------------------------------------------------------------------------------
// One wavefront per row i, one lane per candidate: slots 0 .. K-1 are the row's own neighbours, the others the points that list
// i (RN(i)) minus those already among the neighbours.  Writes the row's candidates (column, or -1 for a slot that holds
// nothing) at i K + rn_ptr[i] and the number of survivors to deg[i].  (k_umap_union_raw's layout with another weight.)
__global__ void __launch_bounds__(256) k_tsne_joint_raw(int n, int K, const int32_t *__restrict__ nn,
                                                        const double *__restrict__ cond, const int *__restrict__ rn_ptr,
                                                        const int32_t *__restrict__ rn_idx, int32_t *__restrict__ raw_col,
                                                        float *__restrict__ raw_w, int *__restrict__ deg)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;                                          // (wave-uniform)
    const int r0 = rn_ptr[i], L = K + (rn_ptr[i + 1] - r0);
    const size_t base = (size_t)i * K + r0;
    const int32_t *ni = nn + (size_t)i * K;
    const double two_n = 2.0 * (double)n;
    int count = 0;
    for (int s0 = 0; s0 < L; s0 += 64) {
        const int s = s0 + lane;
        bool valid = false;
        if (s < L) {
            int j;
            double a = 0.0;
            if (s < K) {
                j = ni[s];
                a = cond[(size_t)i * K + s];
                valid = true;
            } else {
                j = rn_idx[r0 + (s - K)];
                valid = j != i;
                for (int p = 0; p < K && valid; ++p) valid = ni[p] != j;
            }
            float wf = 0.0f;
            if (valid) {
                double b = 0.0;
                const int32_t *nj = nn + (size_t)j * K;
                for (int q = 0; q < K; ++q)
                    if (nj[q] == i) {
                        b = cond[(size_t)j * K + q];
                        break;
                    }
                wf = (float)((a + b) / two_n);                   // a + b commutes: row j computes the same bits
                valid = wf > 0.0f;
            }
            raw_col[base + s] = valid ? j : -1;
            raw_w[base + s] = wf;
        }
        count += __popcll(__ballot(valid));
    }
    if (lane == 0) deg[i] = count;
}

// rank by counting (as k_umap_union_sort): the columns of a row are distinct, so an entry's place is the number of smaller ones
__global__ void __launch_bounds__(256) k_tsne_joint_sort(int n, int K, const int *__restrict__ rn_ptr,
                                                         const int32_t *__restrict__ raw_col, const float *__restrict__ raw_w,
                                                         const int *__restrict__ rowptr, int32_t *__restrict__ col,
                                                         float *__restrict__ w, unsigned int *__restrict__ stats)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int r0 = rn_ptr[i], L = K + (rn_ptr[i + 1] - r0);
    const size_t base = (size_t)i * K + r0;
    const int out = rowptr[i];
    for (int s = lane; s < L; s += 64) {
        const int j = raw_col[base + s];
        if (j < 0) continue;
        int rank = 0;
        for (int t = 0; t < L; ++t) {
            const int jt = raw_col[base + t];
            rank += (jt >= 0 && jt < j) ? 1 : 0;
        }
        col[out + rank] = j;
        w[out + rank] = raw_w[base + s];
    }
    if (lane == 0) atomicMax(&stats[0], (unsigned int)(rowptr[i + 1] - out));
}

// ---- T4: the layout ---------------------------------------------------------------------------------------------------------------
// |d|^2 in f32: the first square, then fmaf over the other coordinates.  q = 1 / (1 + |d|^2) is v_rcp_f32 of it (one f32 step of
// error; the criterion is a tolerance).
template <int C>
__device__ __forceinline__ float sqdist(const float (&d)[C])
{
    float s = d[0] * d[0];
#pragma unroll
    for (int c = 1; c < C; ++c) s = __fmaf_rn(d[c], d[c], s);
    return s;
}

// the fp64 sum of 256 values, one per thread, in a fixed tree; every thread returns it
__device__ __forceinline__ double block_sum_256(double v, double *red)
{
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    return red[0];
}

// Thread (blockIdx.x, threadIdx.x) owns point i and walks j over chunk blockIdx.y of the j axis in ascending order; the chunk
// goes through an LDS tile that every lane reads at the same address.  Accumulates sum q^2 (y_i - y_j) and sum q in f32, j = i
// left out, and writes them to part[(c S + s) n + i] (c = C: the q sum); the workgroup's q sums meet in fp64 in zpart.
template <int C>
__global__ void __launch_bounds__(kRepThreads) k_tsne_repulse(int n, int chunk, const float *__restrict__ Y,
                                                              float *__restrict__ part, double *__restrict__ zpart)
{
    constexpr int CP = C == 2 ? 2 : 4;
    __shared__ __attribute__((aligned(16))) float tile[kRepThreads * CP];
    __shared__ double red[kRepThreads];
    const int i = blockIdx.x * kRepThreads + threadIdx.x;
    const int s = blockIdx.y, S = gridDim.y;
    float yi[C], r[C], sq = 0.0f;
#pragma unroll
    for (int c = 0; c < C; ++c) {
        yi[c] = i < n ? Y[(size_t)i * C + c] : 0.0f;
        r[c] = 0.0f;
    }
    const long long jb_ll = (long long)s * chunk;
    const int jb = jb_ll < n ? (int)jb_ll : n;
    const int je = jb_ll + chunk < n ? (int)(jb_ll + chunk) : n;
    for (int j0 = jb; j0 < je; j0 += kRepThreads) {
        __syncthreads();
        {
            const int j = j0 + (int)threadIdx.x;
            if (j < je) {
#pragma unroll
                for (int c = 0; c < C; ++c) tile[threadIdx.x * CP + c] = Y[(size_t)j * C + c];
            }
        }
        __syncthreads();
        const int lim = je - j0 < kRepThreads ? je - j0 : kRepThreads;
#pragma unroll 4
        for (int jj = 0; jj < lim; ++jj) {
            float d[C];
            if constexpr (C == 2) {
                const f32x2 t = *reinterpret_cast<const f32x2 *>(tile + jj * CP);
                d[0] = yi[0] - t.x; d[1] = yi[1] - t.y;
            } else {
                const f32x4 t = *reinterpret_cast<const f32x4 *>(tile + jj * CP);
                d[0] = yi[0] - t.x; d[1] = yi[1] - t.y; d[2] = yi[2] - t.z;
            }
            float q = __builtin_amdgcn_rcpf(1.0f + sqdist<C>(d));
            q = (j0 + jj == i) ? 0.0f : q;
            sq += q;
            const float q2 = q * q;
#pragma unroll
            for (int c = 0; c < C; ++c) r[c] = __fmaf_rn(q2, d[c], r[c]);
        }
    }
    if (i < n) {
#pragma unroll
        for (int c = 0; c < C; ++c) part[((size_t)c * S + s) * n + i] = r[c];
        part[((size_t)C * S + s) * n + i] = sq;
    }
    const double z = block_sum_256(i < n ? (double)sq : 0.0, red);
    if (threadIdx.x == 0) zpart[(size_t)s * gridDim.x + blockIdx.x] = z;
}

// Z from the nz workgroup sums of k_tsne_repulse: thread t adds entries t, t + 256, ... in order, then the fixed tree
__device__ __forceinline__ double z_from_parts(const double *__restrict__ zpart, int nz, double *red)
{
    double acc = 0.0;
    for (int k = threadIdx.x; k < nz; k += 256) acc += zpart[k];
    return block_sum_256(acc, red);
}

// ... and the same sum on the host (mi_tsne_kl_f32)
double z_from_parts_host(const std::vector<double> &zpart)
{
    double red[256];
    for (int t = 0; t < 256; ++t) {
        double acc = 0.0;
        for (size_t k = (size_t)t; k < zpart.size(); k += 256) acc += zpart[k];
        red[t] = acc;
    }
    for (int off = 128; off > 0; off >>= 1)
        for (int t = 0; t < off; ++t) red[t] += red[t + off];
    return red[0];
}

__device__ __forceinline__ int sign_of(float x) { return (x > 0.0f ? 1 : 0) - (x < 0.0f ? 1 : 0); }

// A group of G lanes owns point v = (global thread) / G; lane l of the group takes entries l, l + G, ... of the row in ascending
// order and the G partial sums meet in a butterfly.  Lane c < C of the group then owns component c: it adds the S repulsion
// partials in chunk order, applies the gain / momentum rule and writes U, gains (in place) and Y_{t+1}.
template <int G, int C>
__global__ void __launch_bounds__(256) k_tsne_update(int n, int S, int nz, const uint32_t *__restrict__ rowptr,
                                                     const int32_t *__restrict__ col, const float *__restrict__ P,
                                                     const float *__restrict__ Yin, float *__restrict__ Yout,
                                                     float *__restrict__ U, float *__restrict__ gains,
                                                     const float *__restrict__ part, const double *__restrict__ zpart,
                                                     double *__restrict__ Zout, float exag, float mom, float eta)
{
    __shared__ double red[256];
    // every workgroup forms Z itself: a third kernel doing it once was 7.6 % slower at n = 2638 and 2.4 % faster at n = 50 000
    // (profiles/tsne_z_reduction_ab.json)
    const double Z = z_from_parts(zpart, nz, red);
    if (blockIdx.x == 0 && threadIdx.x == 0) *Zout = Z;
    const int gl = threadIdx.x & (G - 1);
    const int v = (int)(((long long)blockIdx.x * 256 + threadIdx.x) / G);
    if (v >= n) return;                                          // (the whole group leaves; no barrier follows)
    const uint32_t e0 = rowptr[v], e1 = rowptr[v + 1];
    float yi[C], a[C];
    load_y<C>(Yin, v, yi);
#pragma unroll
    for (int c = 0; c < C; ++c) a[c] = 0.0f;
    for (uint32_t E = e0 + gl; E < e1; E += G) {
        float yj[C], d[C];
        load_y<C>(Yin, col[E], yj);
#pragma unroll
        for (int c = 0; c < C; ++c) d[c] = yi[c] - yj[c];
        const float pq = P[E] * __builtin_amdgcn_rcpf(1.0f + sqdist<C>(d));
#pragma unroll
        for (int c = 0; c < C; ++c) a[c] = __fmaf_rn(pq, d[c], a[c]);
    }
#pragma unroll
    for (int off = G / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int c = 0; c < C; ++c) a[c] += __shfl_xor(a[c], off, 64);
    }
    if (gl < C) {
        float attr = a[0], y = yi[0];
#pragma unroll
        for (int c = 1; c < C; ++c) {
            attr = gl == c ? a[c] : attr;
            y = gl == c ? yi[c] : y;
        }
        float rep = 0.0f;
        for (int s = 0; s < S; ++s) rep += part[((size_t)gl * S + s) * n + v];
        const float g = exag * attr - rep / (float)Z;
        const size_t idx = (size_t)v * C + gl;
        float u = U[idx], gn = gains[idx];
        gn = sign_of(g) != sign_of(u) ? gn + 0.2f : gn * 0.8f;
        gn = fmaxf(gn, 0.01f);
        u = mom * u - (eta * gn) * g;
        U[idx] = u;
        gains[idx] = gn;
        Yout[idx] = y + u;
    }
}

template <int G, int C>
void launch_update(int n, int S, int nz, const uint32_t *rowptr, const int32_t *col, const float *P, const float *Yin,
                   float *Yout, float *U, float *gains, const float *part, const double *zpart, double *Zout, float exag,
                   float mom, float eta)
{
    const unsigned blocks = (unsigned)(((long long)n * G + 255) / 256);
    hipLaunchKernelGGL((k_tsne_update<G, C>), dim3(blocks), dim3(256), 0, 0, n, S, nz, rowptr, col, P, Yin, Yout, U, gains,
                       part, zpart, Zout, exag, mom, eta);
}

template <int C>
void launch_repulse(int n, int S, const float *Y, float *part, double *zpart)
{
    const int chunk = (n + S - 1) / S;
    hipLaunchKernelGGL((k_tsne_repulse<C>), dim3((unsigned)((n + kRepThreads - 1) / kRepThreads), (unsigned)S),
                       dim3(kRepThreads), 0, 0, n, chunk, Y, part, zpart);
}

// chunks of the j axis, a function of n alone: the largest power of two <= n / 64, between 1 and 16
int tsne_chunks(int n)
{
    int S = 1;
    while (S < 16 && 2 * S * 64 <= n) S *= 2;
    return S;
}

// ---- KL ----------------------------------------------------------------------------------------------------------------------------
// one thread per row, fp64 in column order: sum_j P_ij log(P_ij Z (1 + |y_i - y_j|^2)), the squared distance in f32 as in T4
template <int C>
__global__ void __launch_bounds__(256) k_tsne_kl(int n, const uint32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
                                                 const float *__restrict__ P, const float *__restrict__ Y, double Z,
                                                 double *__restrict__ rowkl)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    float yi[C];
    load_y<C>(Y, v, yi);
    double sum = 0.0;
    for (uint32_t E = rowptr[v]; E < rowptr[v + 1]; ++E) {
        float yj[C], d[C];
        load_y<C>(Y, col[E], yj);
#pragma unroll
        for (int c = 0; c < C; ++c) d[c] = yi[c] - yj[c];
        const double p = (double)P[E];
        sum += p * log(p * Z * (1.0 + (double)sqdist<C>(d)));
    }
    rowkl[v] = sum;
}

// what T4 and the KL divergence refuse in (n, c, CSR, Y), before any device work
int check_layout_inputs(int n, int c, const int64_t *rowptr, const int32_t *col, const float *P, const float *Y)
{
    if (!rowptr || !Y) return fail(MI_EINVAL, "NULL argument");
    if (n < 2) return fail(MI_EINVAL, "need n >= 2 (got %d)", n);
    if (c != 2 && c != 3) return fail(MI_EUNSUPPORTED, "n_components must be 2 or 3 (got %d)", c);
    if (n > MI_TSNE_MAX_POINTS) return fail(MI_EUNSUPPORTED, "n = %d exceeds %d", n, MI_TSNE_MAX_POINTS);
    if (rowptr[0] != 0) return fail(MI_EINVAL, "rowptr[0] must be 0");
    for (int i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) return fail(MI_EINVAL, "rowptr decreases at row %d", i);
    const int64_t nnz = rowptr[n];
    if (nnz >= (1ll << 31)) return fail(MI_EUNSUPPORTED, "nnz = %lld reaches 2^31", (long long)nnz);
    if (nnz > 0 && (!col || !P)) return fail(MI_EINVAL, "NULL argument");
    for (int i = 0; i < n; ++i)
        for (int64_t e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            if (col[e] < 0 || col[e] >= n) return fail(MI_EINVAL, "row %d: column %d outside [0, %d)", i, col[e], n);
            if (col[e] == i) return fail(MI_EINVAL, "row %d has a diagonal entry", i);
            if (e > rowptr[i] && col[e] <= col[e - 1]) return fail(MI_EINVAL, "row %d: columns are not strictly ascending", i);
            if (!std::isfinite(P[e]) || !(P[e] > 0.0f)) return fail(MI_EINVAL, "row %d: weight of column %d is not finite and positive", i, col[e]);
        }
    const size_t cells = (size_t)n * c;
    for (size_t e = 0; e < cells; ++e)
        if (!std::isfinite(Y[e])) return fail(MI_EINVAL, "Y[%lld, %lld] is not finite", (long long)(e / c), (long long)(e % c));
    return MI_OK;
}

}  // namespace
}  // namespace mi_sa_impl
using namespace mi_sa_impl;

struct mi_tsne_graph {
    int n = 0, dim = 0, K = 0, device = 0, max_degree = 0;
    int stage = 1;                   // 1 = kNN, 2 = calibrated, 3 = joint P built
    double perplexity = 0.0;
    long long nnz = 0;
    DevArray<int32_t> d_nn, d_col;
    DevArray<float> d_d2, d_P;
    DevArray<double> d_beta, d_cond;
    DevArray<int> d_ptr;
};

extern "C" {

int mi_tsne_destroy(mi_tsne_graph *g)
{
    if (!g) return MI_OK;
    (void)hipSetDevice(g->device);
    delete g;
    return MI_OK;
}

int mi_tsne_knn_f32(const float *X, int n, int dim, double perplexity, int device, mi_tsne_graph **out, float *out_kernel_ms)
{
    if (!X || !out) return fail(MI_EINVAL, "NULL argument");
    if (n < 2 || dim < 1 || dim > 64) return fail(MI_EINVAL, "need n >= 2 and 1 <= dim <= 64 (got n=%d dim=%d)", n, dim);
    if (!(perplexity >= MI_TSNE_MIN_PERPLEXITY && perplexity <= MI_TSNE_MAX_PERPLEXITY))
        return fail(MI_EINVAL, "need %g <= perplexity <= %g (got %g)", MI_TSNE_MIN_PERPLEXITY, MI_TSNE_MAX_PERPLEXITY, perplexity);
    const int K = (int)std::floor(3.0 * perplexity);
    if (K > n - 1) return fail(MI_EINVAL, "perplexity is too large: floor(3 * %g) = %d neighbours, n - 1 = %d", perplexity, K, n - 1);
    if (n > MI_TSNE_MAX_POINTS) return fail(MI_EUNSUPPORTED, "n = %d exceeds %d", n, MI_TSNE_MAX_POINTS);
    const int rc0 = guarded([&]() -> int { return mi_snn_check_points(X, n, dim); });
    if (rc0) return rc0;
    MI_TRY(pick_device(device));
    mi_tsne_graph *g = nullptr;
    const int rc = guarded([&]() -> int {
        g = new mi_tsne_graph();
        g->n = n; g->dim = dim; g->K = K; g->device = device; g->perplexity = perplexity;
        DevBufs tmp;
        float *dX = nullptr;
        HIP_TRY(tmp.upload(&dX, X, (size_t)n * dim));
        HIP_TRY(g->d_nn.resize((size_t)n * K));
        HIP_TRY(g->d_d2.resize((size_t)n * K));
        Timer tm;
        MI_TRY(tm.start(0));
        if (dim <= 16) launch_knn_after<16>(dX, n, dim, K, g->d_nn, g->d_d2);
        else if (dim <= 32) launch_knn_after<32>(dX, n, dim, K, g->d_nn, g->d_d2);
        else launch_knn_after<64>(dX, n, dim, K, g->d_nn, g->d_d2);
        MI_TRY(tm.stop(0, out_kernel_ms));
        return MI_OK;
    });
    if (rc) { mi_tsne_destroy(g); return rc; }
    *out = g;
    return MI_OK;
}

int mi_tsne_fetch_knn(mi_tsne_graph *g, int32_t *nn, float *d2)
{
    if (!g) return fail(MI_EINVAL, "NULL handle");
    HIP_TRY(hipSetDevice(g->device));
    const size_t cells = (size_t)g->n * g->K;
    if (nn) HIP_TRY(hipMemcpy(nn, g->d_nn, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (d2) HIP_TRY(hipMemcpy(d2, g->d_d2, cells * sizeof(float), hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi_tsne_calibrate(mi_tsne_graph *g, float *out_kernel_ms)
{
    if (!g) return fail(MI_EINVAL, "NULL handle");
    HIP_TRY(hipSetDevice(g->device));
    return guarded([&]() -> int {
        const int n = g->n, K = g->K;
        HIP_TRY(g->d_beta.resize((size_t)n));
        HIP_TRY(g->d_cond.resize((size_t)n * K));
        g->stage = 1; g->nnz = 0; g->max_degree = 0;
        Timer tm;
        MI_TRY(tm.start(0));
        hipLaunchKernelGGL(k_tsne_calibrate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, K, std::log(g->perplexity),
                           MI_TSNE_CALIBRATION_STEPS, g->d_d2, g->d_beta, g->d_cond);
        MI_TRY(tm.stop(0, out_kernel_ms));
        g->stage = 2;
        return MI_OK;
    });
}

int mi_tsne_fetch_calibration(mi_tsne_graph *g, double *beta, float *cond)
{
    if (!g) return fail(MI_EINVAL, "NULL handle");
    if (g->stage < 2) return fail(MI_ESTATE, "mi_tsne_fetch_calibration before mi_tsne_calibrate");
    HIP_TRY(hipSetDevice(g->device));
    if (beta) HIP_TRY(hipMemcpy(beta, g->d_beta, (size_t)g->n * sizeof(double), hipMemcpyDeviceToHost));
    if (cond)
        return guarded([&]() -> int {
            std::vector<double> tmp((size_t)g->n * g->K);
            HIP_TRY(hipMemcpy(tmp.data(), g->d_cond, tmp.size() * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t e = 0; e < tmp.size(); ++e) cond[e] = (float)tmp[e];
            return MI_OK;
        });
    return MI_OK;
}

int mi_tsne_symmetrize(mi_tsne_graph *g, float *out_kernel_ms)
{
    if (!g) return fail(MI_EINVAL, "NULL handle");
    if (g->stage < 2) return fail(MI_ESTATE, "mi_tsne_symmetrize before mi_tsne_calibrate");
    HIP_TRY(hipSetDevice(g->device));
    return guarded([&]() -> int {
        const int n = g->n, K = g->K;
        g->d_ptr.reset(); g->d_col.reset(); g->d_P.reset();
        g->stage = 2; g->nnz = 0; g->max_degree = 0;
        DevBufs tmp;
        int *d_cnt = nullptr, *d_rn_ptr = nullptr, *d_cursor = nullptr, *d_deg = nullptr;
        int32_t *d_rn_idx = nullptr, *d_raw_col = nullptr;
        float *d_raw_w = nullptr;
        unsigned int *d_stats = nullptr;
        const size_t raw = 2 * (size_t)n * K;                     // every row: its K neighbours + its reverse list
        HIP_TRY(tmp.alloc(&d_cnt, (size_t)n + 1));
        HIP_TRY(tmp.alloc(&d_rn_ptr, (size_t)n + 1));
        HIP_TRY(tmp.alloc(&d_cursor, (size_t)n + 1));
        HIP_TRY(tmp.alloc(&d_deg, (size_t)n + 1));
        HIP_TRY(tmp.alloc(&d_rn_idx, (size_t)n * K));
        HIP_TRY(tmp.alloc(&d_raw_col, raw));
        HIP_TRY(tmp.alloc(&d_raw_w, raw));
        HIP_TRY(tmp.alloc(&d_stats, 1));
        HIP_TRY(g->d_ptr.resize((size_t)n + 1));
        HIP_TRY(hipMemsetAsync(d_cnt, 0, ((size_t)n + 1) * sizeof(int), 0));
        HIP_TRY(hipMemsetAsync(d_cursor, 0, ((size_t)n + 1) * sizeof(int), 0));
        HIP_TRY(hipMemsetAsync(d_stats, 0, sizeof(unsigned int), 0));
        const unsigned rows = (unsigned)((n + 3) / 4);
        float ms0 = 0.0f, ms1 = 0.0f;
        {
            Timer tm;
            MI_TRY(tm.start(0));
            MI_TRY(mi_snn_reverse_lists_dev(g->d_nn, n, K, d_cnt, d_rn_ptr, d_cursor, d_rn_idx, 0));
            hipLaunchKernelGGL(k_tsne_joint_raw, dim3(rows), dim3(256), 0, 0, n, K, g->d_nn, g->d_cond, d_rn_ptr, d_rn_idx,
                               d_raw_col, d_raw_w, d_deg);
            MI_TRY(mi_scan_exclusive_dev(d_deg, g->d_ptr, n, 0));
            MI_TRY(tm.stop(0, &ms0));
        }
        int nnz = 0;
        HIP_TRY(hipMemcpy(&nnz, g->d_ptr + n, sizeof(int), hipMemcpyDeviceToHost));
        HIP_TRY(g->d_col.resize((size_t)(nnz > 0 ? nnz : 0)));
        HIP_TRY(g->d_P.resize((size_t)(nnz > 0 ? nnz : 0)));
        {
            Timer tm;
            MI_TRY(tm.start(0));
            hipLaunchKernelGGL(k_tsne_joint_sort, dim3(rows), dim3(256), 0, 0, n, K, d_rn_ptr, d_raw_col, d_raw_w, g->d_ptr,
                               g->d_col, g->d_P, d_stats);
            MI_TRY(tm.stop(0, &ms1));
        }
        unsigned int deg_max = 0u;
        HIP_TRY(hipMemcpy(&deg_max, d_stats, sizeof deg_max, hipMemcpyDeviceToHost));
        g->nnz = nnz;
        g->max_degree = (int)deg_max;
        if (out_kernel_ms) *out_kernel_ms = ms0 + ms1;
        g->stage = 3;
        return MI_OK;
    });
}

int mi_tsne_info(const mi_tsne_graph *g, int *n, int *K, int64_t *nnz, int *max_degree)
{
    if (!g) return fail(MI_EINVAL, "NULL handle");
    if (n) *n = g->n;
    if (K) *K = g->K;
    if (nnz) *nnz = g->nnz;
    if (max_degree) *max_degree = g->max_degree;
    return MI_OK;
}

int mi_tsne_fetch_graph(mi_tsne_graph *g, int64_t *rowptr, int32_t *col, float *P)
{
    if (!g) return fail(MI_EINVAL, "NULL handle");
    if (g->stage < 3) return fail(MI_ESTATE, "mi_tsne_fetch_graph before mi_tsne_symmetrize");
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
    if (P && g->nnz) HIP_TRY(hipMemcpy(P, g->d_P, (size_t)g->nnz * sizeof(float), hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi_tsne_layout_f32(int n, int c, const int64_t *rowptr, const int32_t *col, const float *P, const float *Y, const float *U,
                       const float *gains, float eta, float exaggeration, int exaggeration_iters, float momentum0,
                       float momentum1, int momentum_switch_iter, int T, int t0, int center, int device, float *Y_out,
                       float *U_out, float *gains_out, double *Z_out, float *out_kernel_ms)
{
    if (!Y_out) return fail(MI_EINVAL, "NULL argument");
    MI_TRY(check_layout_inputs(n, c, rowptr, col, P, Y));
    if (T < 1 || T > MI_TSNE_MAX_ITERS) return fail(MI_EINVAL, "need 1 <= T <= %d (got %d)", MI_TSNE_MAX_ITERS, T);
    if (t0 < 0 || t0 > INT_MAX - T) return fail(MI_EINVAL, "need 0 <= t0 <= INT_MAX - T (got %d)", t0);
    if (!std::isfinite(eta) || !std::isfinite(exaggeration) || !std::isfinite(momentum0) || !std::isfinite(momentum1))
        return fail(MI_EINVAL, "eta, exaggeration and the momenta must be finite");
    const size_t cells = (size_t)n * c;
    for (size_t e = 0; e < cells; ++e) {
        if (U && !std::isfinite(U[e])) return fail(MI_EINVAL, "U[%lld, %lld] is not finite", (long long)(e / c), (long long)(e % c));
        if (gains && !(std::isfinite(gains[e]) && gains[e] > 0.0f))
            return fail(MI_EINVAL, "gains[%lld, %lld] is not finite and positive", (long long)(e / c), (long long)(e % c));
    }
    MI_TRY(pick_device(device));
    return guarded([&]() -> int {
        const int64_t nnz = rowptr[n];
        std::vector<uint32_t> ptr32((size_t)n + 1);
        for (size_t i = 0; i < ptr32.size(); ++i) ptr32[i] = (uint32_t)rowptr[i];
        std::vector<float> state(cells, 0.0f);
        const int S = tsne_chunks(n);
        const int nb = (n + kRepThreads - 1) / kRepThreads, nz = nb * S;
        DevBufs tmp;
        uint32_t *d_ptr = nullptr;
        int32_t *d_col = nullptr;
        float *d_P = nullptr, *d_Y[2] = {nullptr, nullptr}, *d_U = nullptr, *d_gains = nullptr, *d_part = nullptr;
        double *d_zpart = nullptr, *d_Z = nullptr;
        HIP_TRY(tmp.upload(&d_ptr, ptr32.data(), ptr32.size()));
        HIP_TRY(tmp.upload(&d_col, col, (size_t)nnz));
        HIP_TRY(tmp.upload(&d_P, P, (size_t)nnz));
        HIP_TRY(tmp.upload(&d_Y[0], Y, cells));
        HIP_TRY(tmp.alloc(&d_Y[1], cells));
        HIP_TRY(tmp.upload(&d_U, U ? U : state.data(), cells));
        if (!gains) state.assign(cells, 1.0f);
        HIP_TRY(tmp.upload(&d_gains, gains ? gains : state.data(), cells));
        HIP_TRY(tmp.alloc(&d_part, (size_t)(c + 1) * S * n));
        HIP_TRY(tmp.alloc(&d_zpart, (size_t)nz));
        HIP_TRY(tmp.alloc(&d_Z, 1));
        // lanes per point: the smallest of 16, 32, 64 that holds the mean row length (a function of the graph alone)
        const double mean_deg = (double)nnz / (double)n;
        const int G = mean_deg > 32.0 ? 64 : (mean_deg > 16.0 ? 32 : 16);
        Timer tm;
        MI_TRY(tm.start(0));
        for (int k = 0; k < T; ++k) {
            const int t = t0 + k;
            const float e_t = t < exaggeration_iters ? exaggeration : 1.0f;
            const float m_t = t < momentum_switch_iter ? momentum0 : momentum1;
            const float *in = d_Y[k & 1];
            float *outp = d_Y[(k + 1) & 1];
            if (c == 2) launch_repulse<2>(n, S, in, d_part, d_zpart); else launch_repulse<3>(n, S, in, d_part, d_zpart);
#define MI_TSNE_LAUNCH(GG, CC) \
    launch_update<GG, CC>(n, S, nz, d_ptr, d_col, d_P, in, outp, d_U, d_gains, d_part, d_zpart, d_Z, e_t, m_t, eta)
            if (c == 2) {
                if (G == 64) MI_TSNE_LAUNCH(64, 2); else if (G == 32) MI_TSNE_LAUNCH(32, 2); else MI_TSNE_LAUNCH(16, 2);
            } else {
                if (G == 64) MI_TSNE_LAUNCH(64, 3); else if (G == 32) MI_TSNE_LAUNCH(32, 3); else MI_TSNE_LAUNCH(16, 3);
            }
#undef MI_TSNE_LAUNCH
        }
        MI_TRY(tm.stop(0, out_kernel_ms));
        double Z_last = 0.0;
        HIP_TRY(hipMemcpy(&Z_last, d_Z, sizeof(double), hipMemcpyDeviceToHost));
        // Z = 0: every pair is so far apart that |y_i - y_j|^2 overflowed and q rounded to 0; the step divided by it
        if (!(std::isfinite(Z_last) && Z_last > 0.0))
            return fail(MI_EINVAL, "the normaliser Z of the last iteration is %g: the coordinates are too far apart for f32", Z_last);
        HIP_TRY(hipMemcpy(Y_out, d_Y[T & 1], cells * sizeof(float), hipMemcpyDeviceToHost));
        for (size_t e = 0; e < cells; ++e)
            if (!std::isfinite(Y_out[e])) return fail(MI_EINVAL, "the layout left the range of f32 at Y[%lld, %lld]", (long long)(e / c), (long long)(e % c));
        if (U_out) HIP_TRY(hipMemcpy(U_out, d_U, cells * sizeof(float), hipMemcpyDeviceToHost));
        if (gains_out) HIP_TRY(hipMemcpy(gains_out, d_gains, cells * sizeof(float), hipMemcpyDeviceToHost));
        if (Z_out) *Z_out = Z_last;
        if (center) {                                             // fp64 column means in index order, rounded to f32
            for (int cc = 0; cc < c; ++cc) {
                double sum = 0.0;
                for (int i = 0; i < n; ++i) sum += (double)Y_out[(size_t)i * c + cc];
                const float mean = (float)(sum / (double)n);
                for (int i = 0; i < n; ++i) Y_out[(size_t)i * c + cc] -= mean;
            }
        }
        return MI_OK;
    });
}

int mi_tsne_kl_f32(int n, int c, const int64_t *rowptr, const int32_t *col, const float *P, const float *Y, int device,
                   double *kl, float *out_kernel_ms)
{
    if (!kl) return fail(MI_EINVAL, "NULL argument");
    MI_TRY(check_layout_inputs(n, c, rowptr, col, P, Y));
    MI_TRY(pick_device(device));
    return guarded([&]() -> int {
        const int64_t nnz = rowptr[n];
        std::vector<uint32_t> ptr32((size_t)n + 1);
        for (size_t i = 0; i < ptr32.size(); ++i) ptr32[i] = (uint32_t)rowptr[i];
        const size_t cells = (size_t)n * c;
        const int S = tsne_chunks(n);
        const int nb = (n + kRepThreads - 1) / kRepThreads, nz = nb * S;
        DevBufs tmp;
        uint32_t *d_ptr = nullptr;
        int32_t *d_col = nullptr;
        float *d_P = nullptr, *d_Y = nullptr, *d_part = nullptr;
        double *d_zpart = nullptr, *d_rowkl = nullptr;
        HIP_TRY(tmp.upload(&d_ptr, ptr32.data(), ptr32.size()));
        HIP_TRY(tmp.upload(&d_col, col, (size_t)nnz));
        HIP_TRY(tmp.upload(&d_P, P, (size_t)nnz));
        HIP_TRY(tmp.upload(&d_Y, Y, cells));
        HIP_TRY(tmp.alloc(&d_part, (size_t)(c + 1) * S * n));
        HIP_TRY(tmp.alloc(&d_zpart, (size_t)nz));
        HIP_TRY(tmp.alloc(&d_rowkl, (size_t)n));
        float ms0 = 0.0f, ms1 = 0.0f;
        {
            Timer tm;
            MI_TRY(tm.start(0));
            if (c == 2) launch_repulse<2>(n, S, d_Y, d_part, d_zpart); else launch_repulse<3>(n, S, d_Y, d_part, d_zpart);
            MI_TRY(tm.stop(0, &ms0));
        }
        std::vector<double> zpart((size_t)nz);
        HIP_TRY(hipMemcpy(zpart.data(), d_zpart, zpart.size() * sizeof(double), hipMemcpyDeviceToHost));
        const double Z = z_from_parts_host(zpart);
        {
            Timer tm;
            MI_TRY(tm.start(0));
            const dim3 grid((unsigned)((n + 255) / 256)), block(256);
            if (c == 2) hipLaunchKernelGGL(k_tsne_kl<2>, grid, block, 0, 0, n, d_ptr, d_col, d_P, d_Y, Z, d_rowkl);
            else hipLaunchKernelGGL(k_tsne_kl<3>, grid, block, 0, 0, n, d_ptr, d_col, d_P, d_Y, Z, d_rowkl);
            MI_TRY(tm.stop(0, &ms1));
        }
        std::vector<double> rowkl((size_t)n);
        HIP_TRY(hipMemcpy(rowkl.data(), d_rowkl, rowkl.size() * sizeof(double), hipMemcpyDeviceToHost));
        double sum = 0.0;
        for (int i = 0; i < n; ++i) sum += rowkl[(size_t)i];       // index order
        *kl = sum;
        if (out_kernel_ms) *out_kernel_ms = ms0 + ms1;
        return MI_OK;
    });
}

}  // extern "C"
