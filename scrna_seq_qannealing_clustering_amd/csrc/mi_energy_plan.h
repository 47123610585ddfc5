// mi_energy_plan.h -- how k_energy_dense_mfma (csrc/energy_kernels.hip) cuts its work.  The kernel multiplies the
// S = T (T + 1) / 2 blocks (I, K), K >= I, of the upper block triangle of a T x T grid of 128 x 128 blocks, numbered row
// by row (row I holds K = I .. T - 1), once per tile of 128 states (rtiles of them).  The host cuts that list into
// `pieces` contiguous ranges; a workgroup ("unit") walks one range for one state tile, U = pieces * rtiles units in all.
//   pieces(T, rtiles, cus)       how many ranges: the units should fill whole rounds of the resident workgroups (68 KB of
//                                LDS each: two per CU) with pieces of (nearly) equal length
//   piece_range(S, piece, pieces) the range [s0, s1) of a piece
//   block_of(s, T)               block number -> (I, K)
//   next_block(T, I, K)          the block after (I, K); true when it starts a new row
// Plain C++: the launcher, the kernel and a host program (tests/host/energy_plan_main.cpp) compile the same text.
#pragma once

#if defined(__HIPCC__)
#define MI_EPLAN_FN __host__ __device__ __forceinline__
#else
#define MI_EPLAN_FN inline
#endif

namespace mi_energy_plan {

MI_EPLAN_FN long long blocks(int T) { return (long long)T * (T + 1) / 2; }

// pieces per state tile on a device of `cus` compute units (<= 0: 256)
MI_EPLAN_FN long long pieces(int T, long long rtiles, int cus)
{
    const long long resident = 2LL * (cus > 0 ? cus : 256);
    const long long S = blocks(T);
    long long pieces = 1;
    double best = 0.0;
    for (long long rounds = 1; rounds <= 4; ++rounds) {
        long long p = rounds * resident / rtiles;
        if (p < 1) p = 1;
        if (p > S) p = S;
        const long long units = p * rtiles, longest = (S + p - 1) / p;
        const double fill = (double)(S * rtiles) / (double)(((units + resident - 1) / resident) * resident * longest);
        if (fill > best + 0.02) { best = fill; pieces = p; }
        if (p == S) break;
    }
    return pieces;
}

MI_EPLAN_FN void piece_range(int S, int piece, int pieces, int *s0, int *s1)
{
    *s0 = (int)((long long)S * piece / pieces);
    *s1 = (int)((long long)S * (piece + 1) / pieces);
}

MI_EPLAN_FN void block_of(int s, int T, int *out_I, int *out_K)
{
    int cI = 0;
    while (s >= T - cI) { s -= T - cI; ++cI; }
    *out_I = cI;
    *out_K = cI + s;
}

MI_EPLAN_FN bool next_block(int T, int *I, int *K)
{
    if (++*K == T) { ++*I; *K = *I; return true; }
    return false;
}

}  // namespace mi_energy_plan
