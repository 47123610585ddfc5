// mi_sa_pack.h -- the packed adjacency images the structured kernels read, built on the host from the slot-ELL
// ([slots][D][64] neighbour indices hc and values hv; padding: (the variable itself, +0.0f)).  Plain host code like
// mi_sa_plan.h beside it: no HIP header or type (tests/host/plan_pack_main.cpp runs it under the sanitizers).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace mi_sa_plan {

// CSR (both directions stored, validated by slot_model_facts) -> the slot-ELL: entry k of variable i = 64 t + lane at
// [(t D + k) 64 + lane]
inline void build_slot_ell(const int32_t *rowptr, const int32_t *col, const float *val, int n, int slots, int D,
                           std::vector<uint32_t> &hc, std::vector<float> &hv)
{
    hc.assign((size_t)slots * D * 64, 0u);
    hv.assign((size_t)slots * D * 64, 0.0f);
    for (int t = 0; t < slots; ++t)
        for (int lane = 0; lane < 64; ++lane) {
            const int i = t * 64 + lane;
            for (int k = 0; k < D; ++k) hc[((size_t)t * D + k) * 64 + lane] = (uint32_t)(i < n ? i : 0);
            if (i >= n) continue;
            for (int e = rowptr[i], k = 0; e < rowptr[i + 1]; ++e, ++k) {
                hc[((size_t)t * D + k) * 64 + lane] = (uint32_t)col[e];
                hv[((size_t)t * D + k) * 64 + lane] = val[e];
            }
        }
}

// The register image of a slot: groups of four (neighbour word, value) per lane -- per slot and group [64 lanes][4] words,
// then [64][4] values.  word(j, lane, k): the neighbour word of neighbour j, entry k of the lane; what it is differs by
// kernel: where j's state lives in LDS for K2 (k2_state_word), the byte address of its cell for the others (2 j for K3f's
// 16-bit labels, 4 j for K2p / K2w / K2s).
template <typename WordF>
std::vector<uint32_t> pack_groups_of_four(const std::vector<uint32_t> &hc, const std::vector<float> &hv, int slots, int D, WordF word)
{
    const int G = D / 4;
    std::vector<uint32_t> out((size_t)slots * G * 2 * 64 * 4, 0u);
    for (int t = 0; t < slots; ++t)
        for (int lane = 0; lane < 64; ++lane)
            for (int k = 0; k < D; ++k) {
                const size_t src = ((size_t)t * D + k) * 64 + lane;
                const size_t base = (((size_t)t * G + k / 4) * 2) * 256 + (size_t)lane * 4 + (k & 3);
                out[base] = word(hc[src], lane, k);
                memcpy(&out[base + 256], &hv[src], 4);
            }
    return out;
}

// K2: where the state of variable j lives in LDS (the state starts at LDS address 0): the byte address of its half, its
// byte, or (byte address of its 32-bit word) << 8 | bit
inline uint32_t k2_state_word(uint32_t j, int state_bytes)
{
    return state_bytes == 2 ? 2u * j : (state_bytes == 1 ? j : ((((j >> 5) * 4u) << 8) | (j & 31u)));
}

// K2p's trimmed packing (csrc/sparse_pair_kernels.hip, RW < D): per slot, the groups of four entries that hold a real
// neighbour somewhere -- [64 lanes][4] neighbour words, then [64][4] values -- with the last group cut to the LW = RW - 4 (G - 1)
// entries a row can have: [64][LW] words, then [64][LW] values.  LW = 3 keeps every load 16 / 8 / 4-byte aligned instead:
// [64][4] (three neighbour words, the lane's linear term -- filled in by the caller), [64][2] values, [64][1] value.
// The neighbour word of j is the LDS byte address of its cell, 4 j.
inline std::vector<uint32_t> pack_pair_adjacency(const std::vector<uint32_t> &hc, const std::vector<float> &hv, int slots, int D, int RW)
{
    const int G = D / 4, LW = RW - 4 * (G - 1);
    const size_t slot_words = (size_t)(G - 1) * 512 + (LW == 3 ? 448 : (size_t)LW * 128);
    std::vector<uint32_t> out((size_t)slots * slot_words, 0u);
    for (int t = 0; t < slots; ++t)
        for (int lane = 0; lane < 64; ++lane)
            for (int k = 0; k < RW; ++k) {
                const int g = k / 4, w = g < G - 1 ? 4 : LW;     // entries per lane in this group
                const size_t grp = (size_t)t * slot_words + (size_t)g * 512;
                size_t at_col = grp + (size_t)lane * w + (k & 3), at_val = at_col + (size_t)w * 64;
                if (w == 3) {
                    at_col = grp + (size_t)lane * 4 + (k & 3);
                    at_val = (k & 3) < 2 ? grp + 256 + (size_t)lane * 2 + (k & 3) : grp + 384 + (size_t)lane;
                }
                out[at_col] = 4u * hc[((size_t)t * D + k) * 64 + lane];
                memcpy(&out[at_val], &hv[((size_t)t * D + k) * 64 + lane], 4);
            }
    return out;
}

// K2p's packing with 16-bit neighbour words (csrc/sparse_pair_kernels.hip, N16): the neighbour word of j is still the LDS
// byte address of its cell, 4 j -- below 65 536 for every model of at most 256 slots -- so two share a dword: per slot
// [G / 2 + G][64 lanes][4 dwords], first G / 2 blocks of neighbours (entry k in half k & 1 of dword k / 2 of the lane),
// then G blocks of values (entry k in dword k).  Padding: (self, +0.0).  A slot is 6144 bytes at D = 16 (8448 unpacked).
inline std::vector<uint32_t> pack_pair_adjacency16(const std::vector<uint32_t> &hc, const std::vector<float> &hv, int slots, int D)
{
    const int G = D / 4;
    const size_t slot_words = (size_t)(G / 2 + G) * 256;
    std::vector<uint32_t> out((size_t)slots * slot_words, 0u);
    for (int t = 0; t < slots; ++t)
        for (int lane = 0; lane < 64; ++lane)
            for (int k = 0; k < D; ++k) {
                const size_t src = ((size_t)t * D + k) * 64 + lane;
                const size_t at_nbr = (size_t)t * slot_words + (size_t)(k / 8) * 256 + (size_t)lane * 4 + ((k / 2) & 3);
                const size_t at_val = (size_t)t * slot_words + (size_t)(G / 2 + k / 4) * 256 + (size_t)lane * 4 + (k & 3);
                out[at_nbr] |= (4u * hc[src]) << (16 * (k & 1));
                memcpy(&out[at_val], &hv[src], 4);
            }
    return out;
}

}  // namespace mi_sa_plan
