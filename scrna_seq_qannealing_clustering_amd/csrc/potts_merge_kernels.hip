// potts_merge_kernels.hip -- the merge phase of the Potts annealer (chain 2e): k_potts_merge.
//
// One workgroup per replica, between two launches of K3 / K3f that continue from the replica's labels in HBM:
//   (a) the integer cluster sums W_q, the member counts N_q and the upper triangle of the inter-cluster coupling sums
//       Bq_ab = sum_{l_u = a, l_v = b} vq_uv (fixed point: vq = llrint(S_uv 2^f)) in LDS, with integer atomics -- exact,
//       so the order of the additions does not matter;
//   (b) P proposals "merge cluster b into cluster a", in order, in one wavefront: lane q holds W_q, N_q and the running
//       relabel map of label q in registers; an accepted merge folds row / column b of Bq into a (lane c: entry (a, c));
//   (c) the map applied to the replica's labels in HBM (only when a merge was accepted).
#include "mi_sa_device.h"

namespace mi_sa_impl {
namespace {

constexpr int kMergeThreads = 256;

// index of the pair a < b in the packed upper triangle of a K x K matrix (K (K - 1) / 2 entries)
__device__ __forceinline__ int tri_index(int a, int b, int K)
{
    return a * K - ((a * (a + 1)) >> 1) + (b - a - 1);
}

__device__ __forceinline__ int tri_pair(int a, int b, int K)
{
    return a < b ? tri_index(a, b, K) : tri_index(b, a, K);
}

__global__ void __launch_bounds__(kMergeThreads) k_potts_merge(MergeArgs m)
{
    extern __shared__ __attribute__((aligned(16))) char lds[];
    const int K = m.K, n = m.n, tid = threadIdx.x;
    const int ntri = K * (K - 1) / 2;
    long long *B = reinterpret_cast<long long *>(lds);                        // ntri coupling sums
    int *W = reinterpret_cast<int *>(lds + (size_t)ntri * 8);                 // K cluster sums
    int *N = W + 64;                                                          // K member counts
    int *map = N + 64;                                                        // the relabel map after (b)
    int *acc_all = map + 64;                                                  // merges accepted in (b)
    const int r = blockIdx.x;
    int g = 0, rank = r;                                                      // resolution group, index inside it
    if (m.groups > 1) {
        const int rg = m.R / m.groups;
        g = r / rg;
        rank = r - g * rg;
    }
    const uint32_t gid = m.replica_offset + (uint32_t)rank;
    uint16_t *lab = m.states + (size_t)r * n;

    for (int q = tid; q < ntri; q += kMergeThreads) B[q] = 0;
    if (tid < 64) { W[tid] = 0; N[tid] = 0; }
    // the labels to start from: the caller's initial labels, or the chain's tag-1 words (a call that opens with a merge
    // phase); otherwise the previous launch left them in place
    if (m.src != m.states) {
        for (int i = tid; i < n; i += kMergeThreads) {
            uint32_t v = 0u;
            if ((m.meta[i] >> 31) == 0u)
                v = m.src ? (uint32_t)m.src[(size_t)r * n + i] : chain_word_dev((uint32_t)i, 0u, gid, 1u, m.seed_lo, m.seed_hi) % (uint32_t)K;
            lab[i] = (uint16_t)v;
        }
    }
    __syncthreads();                                                          // (workgroup scope: HBM writes above visible)

    // ---- (a) sums: seat i = thread's position; its D adjacency entries (deg of them real) in slot-ELL order ----
    for (int i = tid; i < n; i += kMergeThreads) {
        const uint32_t meta = m.meta[i];
        if (meta >> 31) continue;                                             // a hole: in no cluster, no couplings
        const int la = lab[i];
        __hip_atomic_fetch_add(&W[la], m.nwq ? m.nwq[i] : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(&N[la], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        const int deg = (int)((meta >> 8) & 0xffffu);
        const size_t base = (size_t)(i >> 6) * m.D * 64 + (i & 63);
        for (int k = 0; k < deg; ++k) {
            const size_t at = base + (size_t)k * 64;
            const int lb = lab[m.ell_col[at]];
            if (la < lb) {                                                    // each unordered edge once: (u, v) with l_u < l_v
                const long long vq = __double2ll_rn(__dmul_rn((double)m.ell_val[at], m.scale));
                __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(&B[tri_index(la, lb, K)]),
                                       (unsigned long long)vq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
        }
    }
    __syncthreads();

    // ---- (b) the proposals, in order, in wavefront 0 ----
    if (tid < 64) {
        const int lane = tid;
        int Wl = lane < K ? W[lane] : 0, Nl = lane < K ? N[lane] : 0, ml = lane;
        const float T = m.temps[m.temps_per_replica ? r : g * m.temps_group_stride + m.sweep_local];
        const double cq = m.cq[g];
        const uint32_t dK = (uint32_t)(K - 1);
        int accepted = 0;
        for (int p0 = 0; p0 < m.proposals; p0 += 64) {
            // lane j draws proposal p0 + j: (a, b) and the threshold -ln(u) T
            uint32_t w[4];
            philox4x32_10((uint32_t)(p0 + lane), m.sweep, gid, 4u, m.seed_lo, m.seed_hi, w);
            const int pa = (int)(w[0] % (uint32_t)K);
            const int pb = (int)(((uint32_t)pa + 1u + w[1] % dK) % (uint32_t)K);
            const float thr = neglog_u(w[2]) * T;
            const int cnt = m.proposals - p0 < 64 ? m.proposals - p0 : 64;
            for (int j = 0; j < cnt; ++j) {
                const int a = __builtin_amdgcn_readlane(pa, j), b = __builtin_amdgcn_readlane(pb, j);
                const int Na = __builtin_amdgcn_readlane(Nl, a), Nb = __builtin_amdgcn_readlane(Nl, b);
                if (Na == 0 || Nb == 0) continue;                             // an empty cluster: no-op
                const long long Wa = __builtin_amdgcn_readlane(Wl, a), Wb = __builtin_amdgcn_readlane(Wl, b);
                // dE = (double)Bq_ab 2^-f + cq (double)(W_a W_b): each product and the sum rounded once, no fma
                const double t1 = __dmul_rn(__ll2double_rn(B[tri_pair(a, b, K)]), m.inv_scale);
                const double t2 = __dmul_rn(cq, __ll2double_rn(Wa * Wb));
                const double dE = __dadd_rn(t1, t2);
                if (!(dE < (double)readlane_f(thr, j))) continue;
                // accept: b's members join a; row / column b of Bq folds into a
                if (lane < K && lane != a && lane != b) {
                    const int ia = tri_pair(a, lane, K), ib = tri_pair(b, lane, K);
                    B[ia] += B[ib];
                    B[ib] = 0;
                }
                if (lane == 0) B[tri_pair(a, b, K)] = 0;
                // (the next proposal reads entries other lanes just wrote: the wave's LDS operations complete in order)
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                if (lane == a) { Wl += (int)Wb; Nl += Nb; }
                if (lane == b) { Wl = 0; Nl = 0; }
                if (ml == b) ml = a;
                ++accepted;
            }
        }
        if (lane < K) map[lane] = ml;
        if (lane == 0) {
            *acc_all = accepted;
            if (accepted) atomicAdd(&m.stats[4], (unsigned long long)accepted);
        }
    }
    __syncthreads();

    // ---- (c) relabel ----
    if (*acc_all == 0) return;
    for (int i = tid; i < n; i += kMergeThreads) {
        if (m.meta[i] >> 31) continue;                                        // holes keep label 0
        const int l = lab[i];
        const int to = map[l];
        if (to != l) lab[i] = (uint16_t)to;
    }
}

}  // namespace

size_t mi_potts_merge_lds_bytes(int K)
{
    return (size_t)K * (K - 1) / 2 * 8 + 3 * 64 * sizeof(int) + 16;
}

int mi_launch_potts_merge(const MergeArgs &m, hipStream_t st)
{
    if (m.K < 2 || m.K > 64) return fail(MI_EUNSUPPORTED, "merge phase: 2 <= K <= 64 (got %d)", m.K);
    hipLaunchKernelGGL(k_potts_merge, dim3(m.R), dim3(kMergeThreads), mi_potts_merge_lds_bytes(m.K), st, m);
    HIP_TRY(hipGetLastError());
    return MI_OK;
}

}  // namespace mi_sa_impl
