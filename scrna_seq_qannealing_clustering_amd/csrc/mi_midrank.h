// mi_midrank.h -- midranks of one vector by the whole workgroup: the one text behind the rank-sum statistics of
// markers_kernels.hip (a gene over the cells) and the Spearman ranks of annot_kernels.hip (a row over the genes), and the
// workgroup sort snn_kernels.hip shares with them.  The pure parts (keys, tie-run search, the network's index arithmetic)
// compile under plain g++: tests/host/midrank_main.cpp runs them under the sanitizers.
//
// The scheme.  The zeros of the vector (both signs) are one tie block whose rank needs no sort: with `neg` negative and
// `zeros` zero entries it holds the ranks neg + 1 .. neg + zeros, doubled midrank 2 neg + zeros + 1.  The non-zeros are
// compacted as (order-preserving u32 key << 32 | id) -- unique 64-bit words, so the sorted array does not depend on the
// order the compaction wrote them in -- padded with ~0 to a power of two and sorted by a bitonic network.  A sorted
// position p finds its tie run [lo, hi) by its neighbours and, inside a run, by binary search; its doubled midrank is
// lo + 1 + hi, plus 2 * zeros for a positive value.  Everything is integers: any thread order gives the same words.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MI_MIDRANK_FN __host__ __device__ __forceinline__
#else
#define MI_MIDRANK_FN inline
#endif

namespace mi_midrank {

MI_MIDRANK_FN bool zero_bits(uint32_t u) { return (u & 0x7fffffffu) == 0u; }

// ascending u32 order == ascending float order over the finite non-zero values (equal floats <=> equal keys); a negative
// has a key < 0x80000000, and no finite value has the key ~0
MI_MIDRANK_FN uint32_t order_key(uint32_t u) { return (u >> 31) ? ~u : (u | 0x80000000u); }

MI_MIDRANK_FN int pow2_at_least(int v)
{
    int p = 0;
    if (v > 0)
        for (p = 1; p < v; p <<= 1) {}
    return p;
}

// The tie run [lo, hi) of sorted position p among the keys S[0 .. nnz) >> 32 (S in LDS or in HBM).
MI_MIDRANK_FN void tie_run(const unsigned long long *S, int p, int nnz, int *lo, int *hi)
{
    const uint32_t key = (uint32_t)(S[p] >> 32);
    *lo = p;
    *hi = p + 1;
    if (p > 0 && (uint32_t)(S[p - 1] >> 32) == key) {                                    // first position with this key, in [0, p - 1]
        int l = 0, r = p - 1;
        while (l < r) {
            const int m = (l + r) >> 1;
            if ((uint32_t)(S[m] >> 32) < key) l = m + 1;
            else r = m;
        }
        *lo = l;
    }
    if (p + 1 < nnz && (uint32_t)(S[p + 1] >> 32) == key) {                              // first position past this key, in [p + 2, nnz]
        int l = p + 2, r = nnz;
        while (l < r) {
            const int m = (l + r) >> 1;
            if ((uint32_t)(S[m] >> 32) <= key) l = m + 1;
            else r = m;
        }
        *hi = l;
    }
}

// Compare t (of P / 2) of the bitonic pass (k, j): the pair (lo, hi = lo | j), ascending when the result is true.
MI_MIDRANK_FN bool sort_pair(int t, int k, int j, int *lo, int *hi)
{
    *lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
    *hi = *lo | j;
    return (*lo & k) == 0;
}

#if defined(__HIPCC__)

// Sorts the P (a power of two, or 0) words of S ascending.  Whole workgroup, any blockDim.x; the caller's barrier has
// published S.  Ends with a barrier.
__device__ __forceinline__ void wg_sort_u64(unsigned long long *S, int P)
{
    const int tid = threadIdx.x, nt = blockDim.x;
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < (P >> 1); t += nt) {
                int lo, hi;
                const bool up = sort_pair(t, k, j, &lo, &hi);
                const unsigned long long x = S[lo], y = S[hi];
                if ((x > y) == up) {
                    S[lo] = y;
                    S[hi] = x;
                }
            }
            __syncthreads();
        }
}

struct Ranked {
    int nnz, zeros;                        // non-zero candidates; zeros of the population
    uint32_t zero_r2;                      // doubled midrank of the zero block
};

// Whole workgroup.  Candidate i of `count` has the value bits bits(i) and the id id(i); the population has `total`
// entries, those that are no non-zero candidate being its zeros (total = count unless the candidates are a sparse
// vector's stored entries).  S: `cap` entries, cap >= pow2_at_least(non-zero candidates); cnt: 2 words of LDS.
// visit(p, entry, lo, hi, r2) is called once per sorted position p by the thread that owns it: entry = S[p], [lo, hi) its
// tie run, r2 its doubled midrank.  No barrier after the visits: the caller's next one frees S and cnt.
template <class Bits, class Id, class Visit>
__device__ __forceinline__ Ranked wg_midranks(int count, Bits bits, Id id, int total, int cap, unsigned long long *S,
                                              uint32_t *cnt, Visit visit)
{
    const int tid = threadIdx.x, nt = blockDim.x, lane = tid & 63;
    if (tid == 0) {
        cnt[0] = 0u;
        cnt[1] = 0u;
    }
    __syncthreads();

    // compaction of the non-zeros (any order: the 64-bit words are unique), count of the negatives
    for (int i0 = 0; i0 < count; i0 += nt) {
        const int i = i0 + tid;
        const uint32_t u = i < count ? bits(i) : 0u;
        const bool nz = !zero_bits(u), ng = nz && (u >> 31);
        const unsigned long long m = __ballot(nz), mn = __ballot(ng);
        if (m) {
            uint32_t base = 0u;
            if (lane == 0) {
                base = atomicAdd(&cnt[0], (uint32_t)__popcll(m));
                if (mn) atomicAdd(&cnt[1], (uint32_t)__popcll(mn));
            }
            base = __shfl(base, 0);
            const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (nz && at < (uint32_t)cap) S[at] = ((unsigned long long)order_key(u) << 32) | (uint32_t)id(i);
        }
    }
    __syncthreads();
    const int nnz = cnt[0] < (uint32_t)cap ? (int)cnt[0] : cap;                          // (a stored zero is a zero)
    const uint32_t neg = cnt[1];
    const int P = pow2_at_least(nnz);                                                    // the sort covers the non-zeros only
    for (int p = nnz + tid; p < P; p += nt) S[p] = ~0ull;                                // (sorts last: no finite key is ~0)
    __syncthreads();
    wg_sort_u64(S, P);

    const Ranked out = {nnz, total - nnz, 2u * neg + (uint32_t)(total - nnz) + 1u};
    for (int p = tid; p < nnz; p += nt) {
        const unsigned long long e = S[p];
        int lo, hi;
        tie_run(S, p, nnz, &lo, &hi);
        visit(p, e, lo, hi, (uint32_t)(lo + 1 + hi) + ((e >> 63) ? 2u * (uint32_t)out.zeros : 0u));
    }
    return out;
}

#endif  // __HIPCC__

}  // namespace mi_midrank
