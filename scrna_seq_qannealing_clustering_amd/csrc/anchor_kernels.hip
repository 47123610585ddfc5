// anchor_kernels.hip -- anchor-based label and feature transfer on MI355X (gfx950): Seurat v4's FindTransferAnchors
// (FindAnchorPairs, ScoreAnchors) and TransferData (FindWeights, the weighted prediction) as this package specifies them.
// C ABI: include/mi_anchors.h.  Specification: DESIGN.md section 5d ("chain A"), restated in numpy by tests/anchor_reference.py.
//
// The reference's assessment notebook ends with FindTransferAnchors + MapQuery(refdata = list(celltype.l1, celltype.l2,
// predicted_ADT = "ADT")) (R/pbmc3k/Pbmc3k_assess_QA_clusters.Rmd:210-237); this file is that step.  The kNN tables are chain
// Q1's (mi_query_knn_dev, mapping_kernels.hip).  Everything after them is integer or fp64 work on small rows: no atomics, one
// order per list and per sum, so two calls return the same bits.
#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/mi_anchors.h"
#include "../../include/mi_umap.h"
#include "mi_umap_shared.h"

namespace mi_sa_impl {
namespace {

constexpr int kMaxK = 64;                 // Q1's limit on every table's width; a mutual mask is one 64-bit word

// ---- A2: mutual pairs -------------------------------------------------------------------------------------------------------
// One thread per cell of the side `A` (n_a cells, its table AB into the other side, the other side's table BA back).
// mask bit p <=> AB[i, p] is mutual: i occurs in BA[AB[i, p], :ka].  The reference side keeps mask and count (the anchor list);
// the query side keeps the count (the anchors-by-query-cell lists).
__global__ void __launch_bounds__(256) k_anchor_pairs_count(int n_a, int K, int ka, const int32_t *__restrict__ AB,
                                                            const int32_t *__restrict__ BA,
                                                            unsigned long long *__restrict__ mask, int *__restrict__ count,
                                                            int *__restrict__ flag)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_a) return;
    unsigned long long mk = 0;
    for (int p = 0; p < ka; ++p) {
        const int32_t *back = BA + (size_t)AB[(size_t)i * K + p] * K;
        bool hit = false;
        for (int j = 0; j < ka; ++j) hit |= back[j] == i;
        if (hit) mk |= 1ull << p;
    }
    if (mask) mask[i] = mk;
    count[i] = __popcll(mk);
    if (flag) flag[i] = mk != 0;
}

// ordered compaction: reference cell r writes its anchors at ptr[r] .., by q's rank in RQ[r]
__global__ void __launch_bounds__(256) k_anchor_pairs_fill(int n, int K, const int32_t *__restrict__ RQ,
                                                           const unsigned long long *__restrict__ mask,
                                                           const int *__restrict__ ptr, int2 *__restrict__ pairs)
{
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= n) return;
    unsigned long long mk = mask[r];
    int o = ptr[r];
    while (mk) {
        const int p = __ffsll(mk) - 1;
        mk &= mk - 1;
        pairs[o++] = make_int2(r, RQ[(size_t)r * K + p]);
    }
}

// the anchors of query cell q in anchor-list order (ascending r: q has one anchor per reference cell at most), as indices
// into the anchor list; U[upos[q]] = q for every query cell with an anchor
__global__ void __launch_bounds__(256) k_anchor_query_fill(int m, int K, int ka, const int32_t *__restrict__ QR,
                                                           const int32_t *__restrict__ RQ,
                                                           const unsigned long long *__restrict__ rmask,
                                                           const int *__restrict__ rptr, const int *__restrict__ qptr,
                                                           const int *__restrict__ upos, int32_t *__restrict__ qanchor,
                                                           int32_t *__restrict__ U)
{
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    const int cnt = qptr[q + 1] - qptr[q];
    if (cnt == 0) return;
    U[upos[q]] = q;
    int last = -1;
    for (int s = 0; s < cnt; ++s) {
        int best = INT_MAX, best_p = 0;
        for (int j = 0; j < ka; ++j) {
            const int r = QR[(size_t)q * K + j];
            if (r <= last || r >= best) continue;
            for (int p = 0; p < ka; ++p)
                if (RQ[(size_t)r * K + p] == q) { best = r; best_p = p; }
        }
        if (best == INT_MAX) return;                                 // (cannot happen: cnt counted these very pairs)
        qanchor[qptr[q] + s] = rptr[best] + __popcll(rmask[best] & ((1ull << best_p) - 1ull));
        last = best;
    }
}

// ---- A3: shared neighbours --------------------------------------------------------------------------------------------------
// One wavefront per anchor, four per workgroup.  The ids of S_r and S_q lie in LDS, each set as its two halves: reference
// cells (< n) and query cells (n + .): a reference id can only meet a reference id, so lane e compares RR[r, e] against the ks
// entries of QR[q] and RQ[r, e] against those of QQ[q] (every lane reads the same LDS address: a broadcast).  The ids within a
// list are distinct, so the hits count the intersection exactly.
__global__ void __launch_bounds__(256) k_anchor_score(int A, int K, int ks, const int2 *__restrict__ pairs,
                                                      const int32_t *__restrict__ RR, const int32_t *__restrict__ RQ,
                                                      const int32_t *__restrict__ QR, const int32_t *__restrict__ QQ,
                                                      int32_t *__restrict__ raw)
{
    __shared__ int32_t s_id[4][4][kMaxK];                         // [wave][RR, RQ, QR, QQ][entry]
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int a = blockIdx.x * 4 + w;
    const bool live = a < A && lane < ks;
    if (live) {
        const int2 rq = pairs[a];
        s_id[w][0][lane] = RR[(size_t)rq.x * K + lane];
        s_id[w][1][lane] = RQ[(size_t)rq.x * K + lane];
        s_id[w][2][lane] = QR[(size_t)rq.y * K + lane];
        s_id[w][3][lane] = QQ[(size_t)rq.y * K + lane];
    }
    __syncthreads();
    int c = 0;
    if (live) {
        const int x = s_id[w][0][lane], y = s_id[w][1][lane];
        bool hx = false, hy = false;
        for (int j = 0; j < ks; ++j) {
            hx |= s_id[w][2][j] == x;
            hy |= s_id[w][3][j] == y;
        }
        c = (int)hx + (int)hy;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if (a < A && lane == 0) raw[a] = c;
}

// ---- A4: the rows of Q[U] ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_anchor_gather(const float *__restrict__ Q, int dim, const int32_t *__restrict__ U,
                                                       long long cells, float *__restrict__ out)
{
    for (long long e = blockIdx.x * 256ll + threadIdx.x; e < cells; e += (long long)gridDim.x * 256)
        out[e] = Q[(size_t)U[e / dim] * dim + e % dim];
}

// ---- A5: anchor weights -----------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_anchor_weight_count(int m, int kw, const int32_t *__restrict__ WN,
                                                             const int32_t *__restrict__ U, const int *__restrict__ qptr,
                                                             int *__restrict__ wcnt)
{
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= m) return;
    int len = 0;
    for (int i = 0; i < kw; ++i) {
        const int u = U[WN[(size_t)c * kw + i]];
        len += qptr[u + 1] - qptr[u];
    }
    wcnt[c] = len;
}

// One wavefront per query cell c.  Lane i owns neighbour i of the row: its anchors land at the exclusive prefix of the lanes'
// counts, which is the row order (i ascending, then anchor-list order).  The unnormalised weights lie in LDS (at most
// kw * ka doubles); lane 0 adds them up in row order, every lane divides its share.
__global__ void __launch_bounds__(64) k_anchor_weights(int kw, double den, const int32_t *__restrict__ WN,
                                                       const float *__restrict__ WD, const int32_t *__restrict__ U,
                                                       const int *__restrict__ qptr, const int32_t *__restrict__ qanchor,
                                                       const double *__restrict__ score, const int *__restrict__ wptr,
                                                       int32_t *__restrict__ out_anchor, double *__restrict__ out_w)
{
    extern __shared__ double s_w[];
    __shared__ double s_sum;
    const int c = blockIdx.x, lane = threadIdx.x;
    const bool live = lane < kw;
    const int base = wptr[c], len = wptr[c + 1] - base;
    const double dk = (double)WD[(size_t)c * kw + kw - 1];
    const int u = live ? U[WN[(size_t)c * kw + lane]] : 0;
    const int first = live ? qptr[u] : 0, cnt = live ? qptr[u + 1] - first : 0;
    int inc = cnt;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(inc, off, 64);
        if (lane >= off) inc += t;
    }
    const int at = inc - cnt;
    if (cnt > 0) {
        const double ratio = dk > 0.0 ? (double)WD[(size_t)c * kw + lane] / dk : 0.0;
        for (int j = 0; j < cnt; ++j) {
            const int a = qanchor[first + j];
            const double t = (1.0 - ratio) * score[a];
            s_w[at + j] = -expm1(-t / den);
            out_anchor[base + at + j] = a;
        }
    }
    __syncthreads();
    if (lane == 0) {
        // row order, with Neumaier's compensation: a plain sum of up to kw * ka terms is off by that many roundings, and the
        // normalised row would miss 1 by as much (5 ulp at 160 terms); this total is within an ulp of the exact one
        double s = 0.0, comp = 0.0;
        for (int e = 0; e < len; ++e) {
            const double x = s_w[e], t = s + x;
            comp += fabs(s) >= fabs(x) ? (s - t) + x : (x - t) + s;
            s = t;
        }
        s_sum = s + comp;
    }
    __syncthreads();
    const double s = s_sum;
    for (int e = lane; e < len; e += 64) out_w[base + e] = s > 0.0 ? s_w[e] / s : 0.0;
}

// ---- A6: prediction ---------------------------------------------------------------------------------------------------------
// One wavefront per query cell: the row's weights and its anchors' class codes in LDS, lane l sums classes l, l + 64, ... over
// the row in row order and keeps its best (classes ascend in a lane: a strict > keeps the smaller on a tie); then the wave's.
__global__ void __launch_bounds__(64) k_anchor_predict_labels(int L, int cap, const int *__restrict__ wptr,
                                                              const int32_t *__restrict__ wanchor,
                                                              const double *__restrict__ weight, const int2 *__restrict__ pairs,
                                                              const int32_t *__restrict__ labels, int32_t *__restrict__ label,
                                                              double *__restrict__ score, double *__restrict__ scores)
{
    extern __shared__ double s_w[];                               // cap doubles, then cap codes
    int32_t *s_code = reinterpret_cast<int32_t *>(s_w + cap);
    const int c = blockIdx.x, lane = threadIdx.x;
    const int base = wptr[c], len = wptr[c + 1] - base;
    for (int e = lane; e < len; e += 64) {
        s_w[e] = weight[base + e];
        s_code[e] = labels[pairs[wanchor[base + e]].x];
    }
    __syncthreads();
    double best = 0.0;
    int best_l = INT_MAX;
    for (int l = lane; l < L; l += 64) {
        double s = 0.0;
        for (int e = 0; e < len; ++e)
            if (s_code[e] == l) s += s_w[e];
        if (scores) scores[(size_t)c * L + l] = s;
        if (s > best) { best = s; best_l = l; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ob = __shfl_xor(best, off, 64);
        const int ol = __shfl_xor(best_l, off, 64);
        if (ob > best || (ob == best && ol < best_l)) { best = ob; best_l = ol; }
    }
    if (lane == 0) {
        label[c] = best > 0.0 ? best_l : -1;
        score[c] = best > 0.0 ? best : 0.0;
    }
}

// One workgroup per query cell, lanes across the features: the row's weights and reference cells in LDS once, then
// pred[c, f] = f32(sum_a w_a * (double)refdata[r_a, f]) in row order (coalesced across f)
__global__ void __launch_bounds__(256) k_anchor_predict_features(int F, int cap, const int *__restrict__ wptr,
                                                                 const int32_t *__restrict__ wanchor,
                                                                 const double *__restrict__ weight,
                                                                 const int2 *__restrict__ pairs,
                                                                 const float *__restrict__ refdata, float *__restrict__ pred)
{
    extern __shared__ double s_w[];                               // cap doubles, then cap reference cells
    int32_t *s_r = reinterpret_cast<int32_t *>(s_w + cap);
    const int c = blockIdx.x;
    const int base = wptr[c], len = wptr[c + 1] - base;
    for (int e = threadIdx.x; e < len; e += blockDim.x) {
        s_w[e] = weight[base + e];
        s_r[e] = pairs[wanchor[base + e]].x;
    }
    __syncthreads();
    for (int f = threadIdx.x; f < F; f += blockDim.x) {
        double acc = 0.0;
        for (int e = 0; e < len; ++e) acc += s_w[e] * (double)refdata[(size_t)s_r[e] * F + f];
        pred[(size_t)c * F + f] = (float)acc;
    }
}

unsigned blocks256(long long items) { return (unsigned)((items + 255) / 256); }

}  // namespace
}  // namespace mi_sa_impl
using namespace mi_sa_impl;

struct mi_anchors {
    int n = 0, m = 0, dim = 0, K = 0, ka = 0, ks = 0, device = 0;
    int A = 0, nU = 0, kw = 0;
    int stage = 1;                       // 1 = anchors found, 2 = scores set, 3 = weights
    long long nnz = 0;
    float ms[MI_ANCHORS_PASSES] = {};
    DevArray<float> d_X;                 // the (normalised) points, R then Q
    DevArray<int32_t> d_RR, d_RQ, d_QR, d_QQ;
    DevArray<unsigned long long> d_rmask;
    DevArray<int> d_rptr, d_qptr;        // anchors by reference cell (the list itself) and by query cell
    DevArray<int2> d_pairs;
    DevArray<int32_t> d_raw, d_qanchor, d_U;
    DevArray<double> d_score;
    DevArray<int32_t> d_WN;              // A4
    DevArray<float> d_WD;
    DevArray<int> d_wptr;                // A5
    DevArray<int32_t> d_wanchor;
    DevArray<double> d_weight;

    int cap() const { return kw * ka; }  // the longest weight row
    int64_t bytes() const
    {
        return (int64_t)(d_X.count * sizeof(float) + (d_RR.count + d_RQ.count + d_QR.count + d_QQ.count) * sizeof(int32_t) +
                         d_rmask.count * sizeof(unsigned long long) + (d_rptr.count + d_qptr.count + d_wptr.count) * sizeof(int) +
                         d_pairs.count * sizeof(int2) +
                         (d_raw.count + d_qanchor.count + d_U.count + d_WN.count + d_wanchor.count) * sizeof(int32_t) +
                         (d_score.count + d_weight.count) * sizeof(double) + d_WD.count * sizeof(float));
    }
};

namespace {

int on_anchors(mi_anchors *a, int stage, const char *what)
{
    if (!a) return fail(MI_EINVAL, "NULL handle");
    if (a->stage < stage)
        return fail(MI_ESTATE, "%s before %s", what, stage == 2 ? "mi_anchors_set_scores" : "mi_anchors_weights");
    HIP_TRY(hipSetDevice(a->device));
    return MI_OK;
}

}  // namespace

extern "C" {

int mi_anchors_destroy(mi_anchors *a)
{
    if (!a) return MI_OK;
    (void)hipSetDevice(a->device);
    delete a;
    return MI_OK;
}

int mi_anchors_find_f32(const float *R, int n, const float *Q, int m, int dim, int k_anchor, int k_score, int l2_norm,
                        int device, mi_anchors **out, float *out_kernel_ms)
{
    if (!R || !Q || !out) return fail(MI_EINVAL, "NULL argument");
    if (n < 2 || m < 2 || dim < 1 || dim > 64)
        return fail(MI_EINVAL, "need n >= 2, m >= 2 and 1 <= dim <= 64 (got n=%d m=%d dim=%d)", n, m, dim);
    const int K = k_anchor > k_score ? k_anchor : k_score;
    if (k_anchor < 2 || k_score < 1 || K > kMaxK || K > n || K > m)
        return fail(MI_EINVAL, "need 2 <= k_anchor, 1 <= k_score and max(k_anchor, k_score) <= min(n, m, 64) (got k_anchor=%d "
                    "k_score=%d n=%d m=%d)", k_anchor, k_score, n, m);
    if (l2_norm != 0 && l2_norm != 1) return fail(MI_EINVAL, "l2_norm must be 0 or 1 (got %d)", l2_norm);
    if (n > MI_UMAP_MAX_POINTS || m > MI_UMAP_MAX_POINTS)
        return fail(MI_EUNSUPPORTED, "n = %d or m = %d exceeds %d", n, m, MI_UMAP_MAX_POINTS);
    if (((long long)n + m) * K >= (1ll << 30))
        return fail(MI_EUNSUPPORTED, "(n + m) * K = %lld reaches 2^30", ((long long)n + m) * K);
    const size_t rcells = (size_t)n * dim, qcells = (size_t)m * dim;
    std::vector<float> both;                                      // A0: R then Q, as the search sees them
    const int rc0 = guarded([&]() -> int {
        both.assign(R, R + rcells);
        both.insert(both.end(), Q, Q + qcells);
        for (size_t e = 0; e < both.size(); ++e)
            if (!std::isfinite(both[e]))
                return fail(MI_EINVAL, "%s[%lld, %lld] is not finite", e < rcells ? "R" : "Q",
                            (long long)((e < rcells ? e : e - rcells) / dim), (long long)(e % dim));
        if (l2_norm) {
            for (int i = 0; i < n + m; ++i) {
                bool any = false;
                for (int c = 0; c < dim; ++c) any |= both[(size_t)i * dim + c] != 0.0f;
                if (!any) return fail(MI_EINVAL, "row %d of %s is all zero: it has no direction to normalise", i < n ? i : i - n, i < n ? "R" : "Q");
            }
            std::vector<float> unit;
            unit_rows(both.data(), n + m, dim, unit);
            both.swap(unit);
        }
        return mi_snn_check_points(both.data(), n + m, dim);
    });
    if (rc0) return rc0;
    MI_TRY(pick_device(device));
    mi_anchors *a = nullptr;
    const int rc = guarded([&]() -> int {
        a = new mi_anchors();
        a->n = n; a->m = m; a->dim = dim; a->K = K; a->ka = k_anchor; a->ks = k_score; a->device = device;
        HIP_TRY(a->d_X.upload(both));
        const float *dR = a->d_X, *dQ = a->d_X.p + rcells;
        HIP_TRY(a->d_RR.resize((size_t)n * K));
        HIP_TRY(a->d_RQ.resize((size_t)n * K));
        HIP_TRY(a->d_QR.resize((size_t)m * K));
        HIP_TRY(a->d_QQ.resize((size_t)m * K));
        {                                                         // A1
            Timer tm;
            MI_TRY(tm.start(0));
            MI_TRY(mi_query_knn_dev(dR, n, dR, n, dim, K, MI_UMAP_EUCLIDEAN, a->d_RR, nullptr));
            MI_TRY(mi_query_knn_dev(dQ, m, dR, n, dim, K, MI_UMAP_EUCLIDEAN, a->d_RQ, nullptr));
            MI_TRY(mi_query_knn_dev(dR, n, dQ, m, dim, K, MI_UMAP_EUCLIDEAN, a->d_QR, nullptr));
            MI_TRY(mi_query_knn_dev(dQ, m, dQ, m, dim, K, MI_UMAP_EUCLIDEAN, a->d_QQ, nullptr));
            MI_TRY(tm.stop(0, &a->ms[0]));
        }
        DevBufs tmp;
        int *d_rcnt = nullptr, *d_qcnt = nullptr, *d_flag = nullptr, *d_upos = nullptr;
        HIP_TRY(tmp.alloc(&d_rcnt, (size_t)n));
        HIP_TRY(tmp.alloc(&d_qcnt, (size_t)m));
        HIP_TRY(tmp.alloc(&d_flag, (size_t)m));
        HIP_TRY(tmp.alloc(&d_upos, (size_t)m + 1));
        HIP_TRY(a->d_rmask.resize((size_t)n));
        HIP_TRY(a->d_rptr.resize((size_t)n + 1));
        HIP_TRY(a->d_qptr.resize((size_t)m + 1));
        int A = 0, A_q = 0, nU = 0;
        {                                                         // A2: count, scan, ordered fill; both sides
            Timer tm;
            MI_TRY(tm.start(0));
            hipLaunchKernelGGL(k_anchor_pairs_count, dim3(blocks256(n)), dim3(256), 0, 0, n, K, k_anchor, a->d_RQ, a->d_QR,
                               a->d_rmask, d_rcnt, (int *)nullptr);
            hipLaunchKernelGGL(k_anchor_pairs_count, dim3(blocks256(m)), dim3(256), 0, 0, m, K, k_anchor, a->d_QR, a->d_RQ,
                               (unsigned long long *)nullptr, d_qcnt, d_flag);
            MI_TRY(mi_scan_exclusive_dev(d_rcnt, a->d_rptr, n, 0));
            MI_TRY(mi_scan_exclusive_dev(d_qcnt, a->d_qptr, m, 0));
            MI_TRY(mi_scan_exclusive_dev(d_flag, d_upos, m, 0));
            HIP_TRY(hipMemcpy(&A, a->d_rptr.p + n, sizeof(int), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(&A_q, a->d_qptr.p + m, sizeof(int), hipMemcpyDeviceToHost));
            HIP_TRY(hipMemcpy(&nU, d_upos + m, sizeof(int), hipMemcpyDeviceToHost));
            if (A != A_q || A < 0 || nU < 0 || nU > m || nU > A)
                return fail(MI_EINVAL, "internal: %d anchors by reference cell, %d by query cell, %d query cells", A, A_q, nU);
            a->A = A; a->nU = nU;
            HIP_TRY(a->d_pairs.resize((size_t)A));
            HIP_TRY(a->d_qanchor.resize((size_t)A));
            HIP_TRY(a->d_U.resize((size_t)nU));
            HIP_TRY(a->d_raw.resize((size_t)A));
            hipLaunchKernelGGL(k_anchor_pairs_fill, dim3(blocks256(n)), dim3(256), 0, 0, n, K, a->d_RQ, a->d_rmask, a->d_rptr,
                               a->d_pairs);
            hipLaunchKernelGGL(k_anchor_query_fill, dim3(blocks256(m)), dim3(256), 0, 0, m, K, k_anchor, a->d_QR, a->d_RQ,
                               a->d_rmask, a->d_rptr, a->d_qptr, d_upos, a->d_qanchor, a->d_U);
            MI_TRY(tm.stop(0, &a->ms[1]));
        }
        {                                                         // A3
            Timer tm;
            MI_TRY(tm.start(0));
            if (A > 0)
                hipLaunchKernelGGL(k_anchor_score, dim3((unsigned)((A + 3) / 4)), dim3(256), 0, 0, A, K, k_score, a->d_pairs,
                                   a->d_RR, a->d_RQ, a->d_QR, a->d_QQ, a->d_raw);
            MI_TRY(tm.stop(0, &a->ms[2]));
        }
        if (out_kernel_ms) *out_kernel_ms = a->ms[0] + a->ms[1] + a->ms[2];
        return MI_OK;
    });
    if (rc) { mi_anchors_destroy(a); return rc; }
    *out = a;
    return MI_OK;
}

int mi_anchors_info(const mi_anchors *a, int *n_anchors, int *n_anchor_queries, int64_t *nnz, int64_t *device_bytes,
                    float *pass_ms)
{
    if (!a) return fail(MI_EINVAL, "NULL handle");
    if (n_anchors) *n_anchors = a->A;
    if (n_anchor_queries) *n_anchor_queries = a->nU;
    if (nnz) *nnz = a->stage >= 3 ? a->nnz : 0;
    if (device_bytes) *device_bytes = a->bytes();
    if (pass_ms)
        for (int p = 0; p < MI_ANCHORS_PASSES; ++p) pass_ms[p] = a->ms[p];
    return MI_OK;
}

int mi_anchors_fetch(mi_anchors *a, int32_t *pairs, int32_t *raw, int32_t *RR, int32_t *RQ, int32_t *QR, int32_t *QQ)
{
    MI_TRY(on_anchors(a, 1, "mi_anchors_fetch"));
    const size_t rt = (size_t)a->n * a->K * sizeof(int32_t), qt = (size_t)a->m * a->K * sizeof(int32_t);
    if (pairs && a->A) HIP_TRY(hipMemcpy(pairs, a->d_pairs, (size_t)a->A * sizeof(int2), hipMemcpyDeviceToHost));
    if (raw && a->A) HIP_TRY(hipMemcpy(raw, a->d_raw, (size_t)a->A * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (RR) HIP_TRY(hipMemcpy(RR, a->d_RR, rt, hipMemcpyDeviceToHost));
    if (RQ) HIP_TRY(hipMemcpy(RQ, a->d_RQ, rt, hipMemcpyDeviceToHost));
    if (QR) HIP_TRY(hipMemcpy(QR, a->d_QR, qt, hipMemcpyDeviceToHost));
    if (QQ) HIP_TRY(hipMemcpy(QQ, a->d_QQ, qt, hipMemcpyDeviceToHost));
    return MI_OK;
}

int mi_anchors_set_scores(mi_anchors *a, const double *score)
{
    MI_TRY(on_anchors(a, 1, "mi_anchors_set_scores"));
    if (!score) return fail(MI_EINVAL, "NULL argument");
    for (int e = 0; e < a->A; ++e)
        if (!(score[e] >= 0.0 && score[e] <= 1.0)) return fail(MI_EINVAL, "score[%d] = %g is not in [0, 1]", e, score[e]);
    a->stage = 1;
    a->d_WN.reset(); a->d_WD.reset(); a->d_wptr.reset(); a->d_wanchor.reset(); a->d_weight.reset();
    a->nnz = 0; a->kw = 0;
    HIP_TRY(a->d_score.upload(score, (size_t)a->A));
    a->stage = 2;
    return MI_OK;
}

int mi_anchors_weights(mi_anchors *a, int k_weight, double sd_weight, float *out_kernel_ms)
{
    MI_TRY(on_anchors(a, 2, "mi_anchors_weights"));
    if (k_weight < 2 || k_weight > kMaxK || k_weight > a->nU)
        return fail(MI_EINVAL, "need 2 <= k_weight <= min(%d, 64), the number of query cells with an anchor (got %d)", a->nU,
                    k_weight);
    if (!std::isfinite(sd_weight) || !(sd_weight > 0.0)) return fail(MI_EINVAL, "sd_weight must be finite and > 0 (got %g)", sd_weight);
    if ((long long)a->m * k_weight * a->ka >= (1ll << 31))
        return fail(MI_EUNSUPPORTED, "m * k_weight * k_anchor = %lld reaches 2^31", (long long)a->m * k_weight * a->ka);
    return guarded([&]() -> int {
        const int m = a->m, dim = a->dim, kw = k_weight, nU = a->nU;
        a->stage = 2;
        const float *dQ = a->d_X.p + (size_t)a->n * dim;
        DevBufs tmp;
        float *d_XU = nullptr;
        int *d_wcnt = nullptr;
        HIP_TRY(tmp.alloc(&d_XU, (size_t)nU * dim));
        HIP_TRY(tmp.alloc(&d_wcnt, (size_t)m));
        HIP_TRY(a->d_WN.resize((size_t)m * kw));
        HIP_TRY(a->d_WD.resize((size_t)m * kw));
        HIP_TRY(a->d_wptr.resize((size_t)m + 1));
        {                                                         // A4
            Timer tm;
            MI_TRY(tm.start(0));
            const long long cells = (long long)nU * dim;
            hipLaunchKernelGGL(k_anchor_gather, dim3(blocks256(cells) < 4096 ? blocks256(cells) : 4096), dim3(256), 0, 0, dQ, dim,
                               a->d_U, cells, d_XU);
            MI_TRY(mi_query_knn_dev(d_XU, nU, dQ, m, dim, kw, MI_UMAP_EUCLIDEAN, a->d_WN, a->d_WD));
            MI_TRY(tm.stop(0, &a->ms[3]));
        }
        {                                                         // A5: count, scan, fill
            Timer tm;
            MI_TRY(tm.start(0));
            hipLaunchKernelGGL(k_anchor_weight_count, dim3(blocks256(m)), dim3(256), 0, 0, m, kw, a->d_WN, a->d_U, a->d_qptr,
                               d_wcnt);
            MI_TRY(mi_scan_exclusive_dev(d_wcnt, a->d_wptr, m, 0));
            int nnz = 0;
            HIP_TRY(hipMemcpy(&nnz, a->d_wptr.p + m, sizeof(int), hipMemcpyDeviceToHost));
            if (nnz < kw || (long long)nnz > (long long)m * kw * a->ka)
                return fail(MI_EINVAL, "internal: %d weight entries for %d rows of at most %d", nnz, m, kw * a->ka);
            HIP_TRY(a->d_wanchor.resize((size_t)nnz));
            HIP_TRY(a->d_weight.resize((size_t)nnz));
            const double bw = 2.0 / sd_weight;
            hipLaunchKernelGGL(k_anchor_weights, dim3((unsigned)m), dim3(64), (size_t)kw * a->ka * sizeof(double), 0, kw, bw * bw,
                               a->d_WN, a->d_WD, a->d_U, a->d_qptr, a->d_qanchor, a->d_score, a->d_wptr, a->d_wanchor,
                               a->d_weight);
            MI_TRY(tm.stop(0, &a->ms[4]));
            a->nnz = nnz;
        }
        a->kw = kw;
        a->stage = 3;
        if (out_kernel_ms) *out_kernel_ms = a->ms[3] + a->ms[4];
        return MI_OK;
    });
}

int mi_anchors_fetch_weights(mi_anchors *a, int64_t *rowptr, int32_t *anchor, double *weight, int32_t *wn, float *wd)
{
    MI_TRY(on_anchors(a, 3, "mi_anchors_fetch_weights"));
    return guarded([&]() -> int {
        const size_t m = (size_t)a->m, nnz = (size_t)a->nnz, cells = m * a->kw;
        if (rowptr) {
            std::vector<int> ptr(m + 1);
            HIP_TRY(hipMemcpy(ptr.data(), a->d_wptr, (m + 1) * sizeof(int), hipMemcpyDeviceToHost));
            for (size_t c = 0; c <= m; ++c) rowptr[c] = ptr[c];
        }
        if (anchor) HIP_TRY(hipMemcpy(anchor, a->d_wanchor, nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (weight) HIP_TRY(hipMemcpy(weight, a->d_weight, nnz * sizeof(double), hipMemcpyDeviceToHost));
        if (wn) HIP_TRY(hipMemcpy(wn, a->d_WN, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
        if (wd) HIP_TRY(hipMemcpy(wd, a->d_WD, cells * sizeof(float), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_anchors_predict_labels(mi_anchors *a, const int32_t *labels, int L, int32_t *label, double *score, double *scores,
                              float *out_kernel_ms)
{
    if (!a) return fail(MI_EINVAL, "NULL handle");
    if (!labels || !label || !score) return fail(MI_EINVAL, "NULL argument");
    if (L < 1) return fail(MI_EINVAL, "need L >= 1 (got %d)", L);
    if (scores && (long long)a->m * L >= (1ll << 31))
        return fail(MI_EUNSUPPORTED, "m * L = %lld reaches 2^31", (long long)a->m * L);
    for (int j = 0; j < a->n; ++j)
        if (labels[j] < -1 || labels[j] >= L) return fail(MI_EINVAL, "labels[%d] = %d is neither -1 nor in [0, %d)", j, labels[j], L);
    MI_TRY(on_anchors(a, 3, "mi_anchors_predict_labels"));
    return guarded([&]() -> int {
        const int m = a->m;
        const size_t dense = scores ? (size_t)m * L : 0;
        DevBufs tmp;
        int32_t *d_labels = nullptr, *d_label = nullptr;
        double *d_score = nullptr, *d_scores = nullptr;
        HIP_TRY(tmp.upload(&d_labels, labels, (size_t)a->n));
        HIP_TRY(tmp.alloc(&d_label, (size_t)m));
        HIP_TRY(tmp.alloc(&d_score, (size_t)m));
        if (scores) HIP_TRY(tmp.alloc(&d_scores, dense));
        Timer tm;
        MI_TRY(tm.start(0));
        hipLaunchKernelGGL(k_anchor_predict_labels, dim3((unsigned)m), dim3(64), (size_t)a->cap() * (sizeof(double) + sizeof(int32_t)),
                           0, L, a->cap(), a->d_wptr, a->d_wanchor, a->d_weight, a->d_pairs, d_labels, d_label, d_score, d_scores);
        MI_TRY(tm.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy(label, d_label, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(score, d_score, (size_t)m * sizeof(double), hipMemcpyDeviceToHost));
        if (scores) HIP_TRY(hipMemcpy(scores, d_scores, dense * sizeof(double), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_anchors_predict_features(mi_anchors *a, const float *refdata, int F, float *pred, float *out_kernel_ms)
{
    if (!a) return fail(MI_EINVAL, "NULL handle");
    if (!refdata || !pred) return fail(MI_EINVAL, "NULL argument");
    if (F < 1) return fail(MI_EINVAL, "need F >= 1 (got %d)", F);
    if ((long long)a->m * F >= (1ll << 31)) return fail(MI_EUNSUPPORTED, "m * F = %lld reaches 2^31", (long long)a->m * F);
    const size_t cells = (size_t)a->n * F;
    for (size_t e = 0; e < cells; ++e)
        if (!std::isfinite(refdata[e])) return fail(MI_EINVAL, "refdata[%lld, %lld] is not finite", (long long)(e / F), (long long)(e % F));
    MI_TRY(on_anchors(a, 3, "mi_anchors_predict_features"));
    return guarded([&]() -> int {
        const int m = a->m;
        DevBufs tmp;
        float *d_ref = nullptr, *d_pred = nullptr;
        HIP_TRY(tmp.upload(&d_ref, refdata, cells));
        HIP_TRY(tmp.alloc(&d_pred, (size_t)m * F));
        const int threads = F >= 256 ? 256 : ((F + 63) / 64) * 64;    // whole wavefronts, lanes across the features
        Timer tm;
        MI_TRY(tm.start(0));
        hipLaunchKernelGGL(k_anchor_predict_features, dim3((unsigned)m), dim3((unsigned)threads),
                           (size_t)a->cap() * (sizeof(double) + sizeof(int32_t)), 0, F, a->cap(), a->d_wptr, a->d_wanchor,
                           a->d_weight, a->d_pairs, d_ref, d_pred);
        MI_TRY(tm.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy(pred, d_pred, (size_t)m * F * sizeof(float), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

}  // extern "C"
