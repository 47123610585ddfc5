// mi_sa_chain_ends.h -- where a chain of the structured anneal kernels (K2 / K2s / K2w / K2p, K3 / K3f) starts and what
// it reports when it ends: the parts of that text that are written once.  Shared here: the Potts initial labels and chain
// out (K3, K3f), the binary initial state (K2s, K2w), the binary closing expression (all four).  Still per kernel: the
// initial state of K2 and K2p and the binary per-lane energy loop ("Chain ends", says why).  The order of the
// fp64 sums IS the specification of the reported energy (tests/chain_ends_reference.py restates it in numpy): energies are
// compared bit for bit across kernel forms, shards and continued runs.  A kernel passes a small lambda that reads or
// writes ITS cell encoding.  None of this runs inside a sweep.
#pragma once

#include "mi_sa_device.h"

namespace mi_sa_impl {

// ------------------------------------------------------------------------------------------------
// binary family
// ------------------------------------------------------------------------------------------------
// Initial state of replica r (random stream gid) on the slots t0, t0 + step, ... (step divides a.slots): a hole
// (lin = +inf) of a padded layout, mi_sa_plan_slot_layout, or a seat past n starts at 0 and its dE = +inf is never
// accepted; every other seat takes the caller's byte, or bit 31 of word t & 3 of the tag-1 Philox block t >> 2.
// store(i, x) writes the kernel's cell.  Returns this wave's sum_j w_j x_j over those slots: a popcount, but on slot
// wslot, whose lanes carry the weights wl (a kernel that takes no weighted model passes -1).
// K2s and K2w start here.  K2 and K2p keep their own text of the same rule: written through this function, with the
// argument block by value, by reference or as scalars, their register figures move (profiles/chain_ends_refactor_ab.json,
// shared_forms_tried).
template <typename StoreF>
__device__ __forceinline__ int binary_initial_state(const EllArgs &a, int r, uint32_t gid, int lane, int t0, int step,
                                                    int wslot, int wl, StoreF store)
{
    const uint8_t *init = static_cast<const uint8_t *>(a.init);
    int S = 0;
    for (int b = 0; b < a.slots / step; ++b) {
        const int t = b * step + t0;
        const int i = t * 64 + lane;
        const bool real = i < a.n && a.lin[i] < INFINITY;
        bool x;
        if (init) {
            x = real && init[(size_t)r * a.n + i] != 0;
        } else {
            uint32_t w[4];
            philox4x32_10((uint32_t)((t >> 2) * 64 + lane), 0u, gid, 1u, a.seed_lo, a.seed_hi, w);
            const int c = t & 3;
            x = real && ((c == 0 ? w[0] : (c == 1 ? w[1] : (c == 2 ? w[2] : w[3]))) >> 31);
        }
        store(i, x);
        S += t == wslot ? (int)wave_sum_i64(x ? (long long)wl : 0ll) : __popcll(__ballot(x));
    }
    return S;
}

// Every kernel of the family sums, per lane with its slots ascending,
//     e = sum over the on-variables i of  lin_i + 0.5 * acc_i,   acc_i = sum over k ascending of val_ik [x_col_ik]
// (the fp64 coefficients when set), then over the lanes by the xor butterfly of wave_sum_f64 (off = 32 ... 1); K2s with
// 2 or 4 wavefronts adds the waves' sums in ascending wave order.  cnt = sum_j w_j x_j, cnt2 = sum_j w_j^2 x_j (both the
// number of on-variables when every weight is 1).  That loop stays in each kernel (shared, it moves register figures of
// K2, K2p and K2w); what follows it is this ONE expression: the uniform pair term (w = 1: cnt (cnt - 1) / 2 pairs)
// and the offset.  (The constants come as scalars: handed the argument block, K2p's register figures move.)
__device__ __forceinline__ double binary_chain_finish(const double *ell_val64, float c_pair, double c_pair64, double offset,
                                                      double e, long long cnt, long long cnt2)
{
    const double cp = ell_val64 ? c_pair64 : (double)c_pair;
    return e + cp * 0.5 * ((double)cnt * (double)cnt - (double)cnt2) + offset;
}

// ------------------------------------------------------------------------------------------------
// Potts family
// ------------------------------------------------------------------------------------------------
// fp64 weighted pair term of the reported energy (chain 2d): c64 / 2 sum_q (W_q^2 - sum_{i in q} w_i^2), returned as this
// lane's share of a wave sum (lane 0 carries the cluster sums); c64 of resolution group grp.  label(i): the label of position i (every lane of the wave
// calls it for the same t).
template <typename LabelF>
__device__ double node_weight_energy(const EllArgs &a, int lane, int grp, LabelF label)
{
    double own = 0.0, tot = 0.0;
    for (int t = 0; t < a.slots; ++t) {
        const double w = a.nw64[t * 64 + lane];
        own -= w * w;
    }
    for (int q = 0; q < a.K; ++q) {
        double s = 0.0;
        for (int t = 0; t < a.slots; ++t) {
            const int i = t * 64 + lane;
            if (label(i) == (uint32_t)q) s += a.nw64[i];        // (0 at holes and past n)
        }
        s = wave_sum_f64(s);
        tot += s * s;
    }
    const double c64 = a.gconst ? a.gconst[grp] : (a.ell_val64 ? a.c_pair64 : (double)a.c_pair);
    return 0.5 * c64 * (own + (lane == 0 ? tot : 0.0));
}

// Initial labels of replica r (random stream gid): a position where nobody sits (bit 31 of meta: past n, or a hole of a
// padded layout, mi_sa_plan_slot_layout / mi_sa_problem_set_absent) holds label 0, is in no cluster and is never
// proposed; every other one takes the caller's label, or word t & 3 of the tag-1 Philox block t >> 2 modulo K.
// store(i, v) writes the kernel's cell and label(i) reads it back.  cnt[q], q < K (64 words): the size of cluster q, or
// for WT its integer weight sum (exact: integer atomics in any order; the wave's LDS operations run in order).
template <bool WT, typename StoreF, typename LabelF>
__device__ __forceinline__ void potts_initial_labels(const EllArgs &a, int r, uint32_t gid, int lane, int *cnt, StoreF store,
                                                     LabelF label)
{
    const uint16_t *init = static_cast<const uint16_t *>(a.init);
    for (int tg = 0; tg * 4 < a.slots; ++tg) {
        uint32_t w[4] = {0u, 0u, 0u, 0u};
        if (!init) philox4x32_10((uint32_t)(tg * 64 + lane), 0u, gid, 1u, a.seed_lo, a.seed_hi, w);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int t = 4 * tg + c;
            if (t >= a.slots) break;
            const int i = t * 64 + lane;
            uint32_t v = 0u;
            if ((a.meta[i] >> 31) == 0u) v = init ? (uint32_t)init[(size_t)r * a.n + i] : (w[c] % (uint32_t)a.K);
            store(i, v);
        }
    }
    int cntv = 0;                                                // lane q: number of variables with label q
    for (int q = 0; q < a.K; ++q) {
        int c = 0;
        for (int t = 0; t < a.slots; ++t)
            c += __popcll(__ballot((a.meta[t * 64 + lane] >> 31) == 0u && label(t * 64 + lane) == (uint32_t)q));
        if (lane == q) cntv = c;
    }
    cnt[lane] = cntv;
    if constexpr (WT) {
        cnt[lane] = 0;
        for (int t = 0; t < a.slots; ++t) {
            const int i = t * 64 + lane;
            if ((a.meta[i] >> 31) == 0u) __hip_atomic_fetch_add(&cnt[label(i)], a.nwq[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
        }
    }
}

// Chain out of replica r (resolution group grp): the labels, and the reported energy -- per lane the edges (i, col) with
// col > i inside one cluster, slots and entries ascending (W per row; the fp64 coefficients when set), then the lane's
// share of the pair term (lane q < K: c / 2 n_q (n_q - 1) from cnt[q]; WT: node_weight_energy), the butterfly of
// wave_sum_f64, and the constant (WT: the group's).  Adds `accepted` to stats[1].  label(i): the label of position i.
template <bool WT, typename LabelF>
__device__ __forceinline__ void potts_chain_out(const EllArgs &a, int r, int grp, int lane, int W, const int *cnt,
                                                unsigned long long accepted, LabelF label)
{
    uint16_t *dst = static_cast<uint16_t *>(a.states) + (size_t)r * a.n;
    double e = 0.0;
    for (int t = 0; t < a.slots; ++t) {
        const int i = t * 64 + lane;
        if (i >= a.n) continue;
        const uint32_t li = label(i);
        dst[i] = (uint16_t)li;
        for (int k = 0; k < W; ++k) {
            const size_t at = ((size_t)t * W + k) * 64 + lane;
            const uint32_t cc = a.ell_col[at];
            const double vv = a.ell_val64 ? a.ell_val64[at] : (double)a.ell_val[at];
            if ((int)cc > i && label((int)cc) == li) e += vv;
        }
    }
    if constexpr (WT) {
        e += node_weight_energy(a, lane, grp, label);
    } else {
        const int cntv = cnt[lane];
        if (lane < a.K) e += (a.ell_val64 ? a.c_pair64 : (double)a.c_pair) * 0.5 * (double)cntv * (double)(cntv - 1);
    }
    e = wave_sum_f64(e);
    if (lane == 0) {
        a.energy[r] = e + (WT && a.gconst ? a.gconst[a.groups + grp] : a.offset);
        atomicAdd(&a.stats[1], accepted);
    }
}

}  // namespace mi_sa_impl
