// sparse_pair_kernels.hip -- K2p: the CSR + uniform-pair anneal with TWO replicas per wavefront (gfx950 only).
//
// Why.  With the accept mask found by fixed-point rounds (sparse_kernels.hip) K2 is bound by the vector-memory
// path: every wavefront re-reads its slot's adjacency (D x 64 x 8 bytes = 8 KB at D = 16) from L2 for every slot of
// every sweep -- 29 TB/s of the ~34.5 TB/s the L2s deliver (profiles/r02_*), 64 B/clk per CU.  The adjacency does
// not depend on the replica, so here a wavefront carries TWO replicas through the same slot: one set of adjacency
// registers, two states, two fields, two thresholds.  L2 traffic per update halves.
//
// State layout: one 32-bit cell per variable in LDS, [half x of replica A | half x of replica B] (0.0 / 1.0), so ONE
// ds_read_b32 per neighbour serves both replicas and v_fma_mix_f32 takes either half as it is (op_sel).  4 bytes per
// variable per wavefront: n <= 4608 keeps 8 wavefronts (16 replicas) per CU.
//
// The chain is K2's (oracle/sa_oracle.c 2b), bit for bit; only models whose every slot is free of internal edges
// (the slot-independent order) take this kernel -- the others run on k_anneal_csr_rank1.
#include "mi_sa_chain_ends.h"

namespace mi_sa_impl {

namespace {

typedef _Float16 half_t;

// phase cycle counters of the sweeping wavefront (`make dbg DBG_FLAGS=-DMI_K2P_PROFILE DBG_NAME=pprof`; perturbs the run)
#ifdef MI_K2P_PROFILE
#define K2P_TICK(var) do { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); const unsigned long long now_ = __builtin_amdgcn_s_memtime(); var += now_ - tick_; tick_ = now_; } while (0)
#else
#define K2P_TICK(var) do { } while (0)
#endif

__device__ __forceinline__ float half_lo(uint32_t w) { return (float)__builtin_bit_cast(half_t, (uint16_t)w); }
__device__ __forceinline__ float half_hi(uint32_t w) { return (float)__builtin_bit_cast(half_t, (uint16_t)(w >> 16)); }

// TW ("threshold wavefront", round 3): the workgroup has a SECOND wavefront that does the part of a sweep which does not
// depend on the state -- the random words (Philox) and the thresholds -ln(u) * T of both replicas -- one group of four
// slots ahead, and hands them over through a two-deep ring in LDS (one ds_write_b64 / ds_read_b64 per slot and lane,
// one s_barrier per group).  Why: with two wavefronts per SIMD the kernel is bound by what ONE wavefront can issue
// (a lone wavefront issues a vector instruction every 5.8 cycles, scripts/ubench_valu.hip; the SIMD could take one every
// 1.5-2), and a third of the instructions of a slot are these thresholds.  A 128-thread workgroup puts its two
// wavefronts on different SIMDs and every SIMD ends up with two sweeping and two threshold wavefronts
// (scripts/probe_placement.hip).  Same chain: the thresholds are the same function of (variable, sweep, replica).
// Priority: the threshold wavefront stays at 0; the sweeping wavefront runs at 3, and in the pipelined forms (N16 = 2) at 3
// or 2, set once per sweep by its hardware wave slot, so that the two sweeping wavefronts of a SIMD lead in turn (PR below).
// WGT: the model carries pair-term weights (mi_sa_problem_set_pair_weights; weighted_slot_sweep): a template switch, so
// that the other models' code is what it was.
// RW < D ("trimmed rows", the name's " r<RW>"): the model's longest row is RW < D entries, so entries RW.. D-1 of every
// lane are padding (self, +0.0) in every slot.  They only ever add fma(+0, x, g) -- the oracle iterates CSR entries, and
// the only effect is the sign of a zero field, which dE < thr cannot see -- so this form neither fetches nor gathers
// them: a.adj4 then holds the trimmed packing (mi_sa.hip, pack_pair_adjacency), whose last group carries LW = RW - 4 (G - 1)
// entries per lane ([64][LW] neighbours, then [64][LW] values; LW = 3: one dwordx4 of three neighbours and the linear
// term, one dwordx2 and one dword of values -- 7936 bytes per slot and wavefront instead of 8448, nine loads as before).
// N16 ("16-bit neighbour words", round 5): a neighbour word is the LDS byte address of a cell, below 65 536 on every model
// of at most 256 slots, so a.adj4 then holds two of them per dword (mi_sa.hip, pack_pair_adjacency16: per slot G / 2 blocks
// of [64 lanes][4 dwords] neighbours, entry k in half k & 1 of dword k / 2, then G such blocks of values; RW < D: the last
// value of a lane, padding in every row, is its linear term) -- six aligned dwordx4 loads and 6144 bytes per slot and
// wavefront at D = 16.  Same chain: the same neighbours in the same order, the same values, the same fma sequence; an
// address costs one v_and_b32 or v_lshrrev_b32 more.  N16 = 1 (D = 32, no threshold wavefront): unpacked at the top of the
// slot from the slot's own registers.  N16 = 2 (TW): the neighbour dwords are fetched TWO slots ahead and the addresses of
// slot t + 1 are unpacked under the gathers of slot t, next to the own-cell terms -- measured against N16 = 1 on the TW
// form: 21.08 against 21.27 ms on the benchmark's model.  The D = 16 form WITHOUT a threshold wavefront keeps the 32-bit
// packing: there the unpack at the top of the slot cost more than the bytes saved (profiles/r05_k2p_nbr16_ab.txt).
// Round 6 takes fixed costs off the sweeping wavefront of the N16 = 2 forms, where every instruction of that wavefront is
// on the critical path (an LDS instruction costs it 12-19 cycles, a vector one 5):
// GR ("group-wide reads"): the lane's own cells of a group of four slots (only that lane writes them, each in its own
// slot) and the group's thresholds are read once after the group's barrier -- two ds_read2st64_b32 (the cells lie 256
// bytes apart) and two ds_read_b128 on one address each, instead of four ds_read_b32 and four ds_read_b64 on eight; the
// threshold wavefront writes two ds_write_b128 instead of four ds_write_b64 (ring: [2 halves][64 lanes][16 bytes] per group,
// the same 2048 bytes).  Slot 0's counted wait proves all four back; slots 1 to 3 wait for nothing but their gathers.
// CY ("carry"; sweeps of six slots and more -- the launcher's choice): the adjacency prefetch runs on over the end of a
// sweep into the next one instead of fetching the last slot again for nothing and filling the pipeline anew (one exposed L2
// round trip and ~25 instructions per sweep).
// All forms: the fp64 energy epilogue requests a slot's indices and values together (two round trips per slot and
// replica instead of 2 D dependent ones).  profiles/r06_k2p_fixed_costs_ab.txt.
template <int D, bool TW, bool WGT = false, int RW = D, int N16 = 0, bool CY = false>
__global__ void __launch_bounds__(TW ? 128 : 64, TW ? 1 : 2) k_anneal_csr_rank1_pair(EllArgs a)
{
    static_assert(RW > D - 4 && RW <= D, "trimmed rows drop part of the last group of four only");
    static_assert(N16 == 0 || !WGT, "the weighted form keeps the 32-bit packing");
    static_assert(N16 != 2 || (TW && D == 16), "the pipelined unpack lives in the threshold-wavefront form's gather window");
    static_assert(!CY || N16 == 2, "the carried prefetch is the pipelined form's");
    extern __shared__ __attribute__((aligned(16))) char lds[];      // cell of variable i at byte 4 i
    const int lane = threadIdx.x & 63;
    const int pair = blockIdx.x;                                    // replicas 2 pair, 2 pair + 1
    const int rA = 2 * pair, rB = 2 * pair + 1;
    if (rA >= a.R) return;
    const bool liveB = rB < a.R;                                    // an odd R leaves the last wavefront one idle seat
    const uint32_t gidA = a.replica_offset + (uint32_t)rA, gidB = gidA + 1u;
    const int n = a.n, slots = a.slots;
    const uint8_t *init = static_cast<const uint8_t *>(a.init);
    uint32_t *cell = reinterpret_cast<uint32_t *>(lds);
    // GR ("group-wide reads", round 6; the N16 = 2 forms): what a group of four slots reads of its lane's own cells and
    // thresholds is read once, after the group's barrier
    // (`make dbg DBG_FLAGS=-DMI_K2P_NO_GROUPREADS` / `-DMI_K2P_NO_CARRY` / `-DMI_K2P_NO_EPI`: the A/B arms without a part)
#ifdef MI_K2P_NO_GROUPREADS
    constexpr bool GR = false;
#else
    constexpr bool GR = N16 == 2;
#endif
    // TW: the ring of thresholds behind the cells: 2 groups x 4 slots x 64 lanes x (thrA, thrB)
    // (GR: a group's 2048 bytes are [2 halves][64 lanes][thrA, thrB of slot 4 g + 2 h, then of slot 4 g + 2 h + 1])
    const uint32_t ring_lane = (uint32_t)slots * 256u + (uint32_t)lane * (GR ? 16u : 8u);

    if constexpr (TW) {
        if (__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) == 1) {
            // ---- the threshold wavefront ----
            uint32_t wa[4], wb[4];
            uint32_t buf = 0;
            for (int s = 0; s < a.num_sweeps; ++s) {
                float TA, TB;
                if (a.temps_per_replica) {
                    TA = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.temps[rA])));
                    TB = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.temps[liveB ? rB : rA])));
                } else {
                    TA = TB = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.temps[s])));
                }
                const uint32_t sw = (uint32_t)s + a.sweep_offset;
#pragma unroll 1
                for (int t = 0; t < slots; t += 4) {
#ifdef MI_K2P_DBG_NOPROD   /* timing only: no random words */
                    for (int c = 0; c < 4; ++c) wa[c] = wb[c] = (uint32_t)(t + c) * 0x9E3779B9u + lane * 77u;
#else
                    philox4x32_10((uint32_t)((t >> 2) * 64 + lane), sw, gidA, 0u, a.seed_lo, a.seed_hi, wa);
                    philox4x32_10((uint32_t)((t >> 2) * 64 + lane), sw, gidB, 0u, a.seed_lo, a.seed_hi, wb);
#endif
                    const uint32_t at = ring_lane + buf;
                    if constexpr (GR) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const f32x2_t t0 = neglog_u2(wa[2 * h], wb[2 * h]) * f32x2_t{TA, TB};
                            const f32x2_t t1 = neglog_u2(wa[2 * h + 1], wb[2 * h + 1]) * f32x2_t{TA, TB};
                            const f32x4 thr = {t0.x, t0.y, t1.x, t1.y};
                            asm volatile("ds_write_b128 %0, %1 offset:%2" :: "v"(at), "v"(thr), "n"(h * 1024) : "memory");
                        }
                    } else
#pragma unroll
                    for (int c = 0; c < 4; ++c) {
                        const f32x2_t thr = neglog_u2(wa[c], wb[c]) * f32x2_t{TA, TB};
                        asm volatile("ds_write_b64 %0, %1 offset:%2" :: "v"(at), "v"(thr), "n"(c * 512) : "memory");
                    }
                    buf ^= 2048u;
                    // group (s, t) is in the ring: the sweeping wavefront passes the same barrier before it reads it, and
                    // passes the NEXT one only after it has read it -- so the buffer written next (the other one) is free
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                }
            }
            return;
        }
    }

    // (pair-term weights, mi_sa_problem_set_pair_weights: SA / SB are sum_j w_j x_j; the one slot whose lanes carry weights
    // other than 1 is swept by a serial loop -- weighted_slot_sweep)
    const int wslot = WGT ? a.wslot : -1;
    const int wl = wslot >= 0 ? a.wgt[lane] : 0;
    int SA = 0, SB = 0;
    for (int tg = 0; tg * 4 < slots; ++tg) {
        uint32_t wa[4] = {0u, 0u, 0u, 0u}, wb[4] = {0u, 0u, 0u, 0u};
        if (!init) {
            philox4x32_10((uint32_t)(tg * 64 + lane), 0u, gidA, 1u, a.seed_lo, a.seed_hi, wa);
            philox4x32_10((uint32_t)(tg * 64 + lane), 0u, gidB, 1u, a.seed_lo, a.seed_hi, wb);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int t = 4 * tg + c;
            if (t >= slots) break;
            const int i = t * 64 + lane;
            bool xa, xb;
            const bool real = i < n && a.lin[i] < INFINITY;         // (+inf linear term = hole of a padded layout: stays 0)
            if (init) {
                xa = real && init[(size_t)rA * n + i] != 0;
                xb = real && liveB && init[(size_t)rB * n + i] != 0;
            } else {
                xa = real && (wa[c] >> 31);
                xb = real && (wb[c] >> 31);
            }
            cell[i] = (xa ? 0x3c00u : 0u) | (xb ? 0x3c000000u : 0u);
            if (WGT && t == wslot) {
                SA += (int)wave_sum_i64(xa ? (long long)wl : 0ll);
                SB += (int)wave_sum_i64(xb ? (long long)wl : 0ll);
            } else {
                SA += __popcll(__ballot(xa));
                SB += __popcll(__ballot(xb));
            }
        }
    }

    constexpr int G = D / 4;                                        // groups of four (neighbour, value) per lane
    constexpr int LW = RW - 4 * (G - 1);                            // entries of the last group (4 unless trimmed)
    constexpr int GC = N16 ? G / 2 : G;                             // dwordx4 blocks of neighbour words per lane
    constexpr int SLOT_BYTES = N16 ? (GC + G) * 1024 : (G - 1) * 2048 + (LW == 3 ? 1792 : LW * 512);   // one slot of the packing
    const __amdgpu_buffer_rsrc_t rs_adj = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint4 *>(a.adj4), 0, slots * SLOT_BYTES, 0x00020000);
    const __amdgpu_buffer_rsrc_t rs_lin = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(a.lin), 0, slots * 256, 0x00020000);
    struct SlotAdj { u32x4 col[GC]; u32x4 val[G]; uint32_t lin; };
    struct NbrPack { u32x4 w[GC]; };                                // N16: the packed neighbour dwords of a slot
    const int lane16 = lane * 16;
    // N16: block b of a slot's [GC + G][64][4] image (constant parts of the offset fold into the 12-bit immediate)
    // a slot past the last one: clamped (fetched for nothing), or -- `wrap`, the carried prefetch: at most five slots ahead
    // in sweeps of six slots and more -- the slot of the NEXT sweep it stands for
    using std::integral_constant;
    using no_wrap = integral_constant<bool, false>;
    auto slot_of = [&](int t, auto wrap) { return t < slots ? t : (decltype(wrap)::value ? t - slots : slots - 1); };
    auto fetch_block16 = [&](int t, int b, auto wrap) {
        return __builtin_amdgcn_raw_buffer_load_b128(rs_adj, lane16 + (b & 3) * 1024, slot_of(t, wrap) * SLOT_BYTES + (b >> 2) * 4096, 0);
    };
    auto fetch_nbr16 = [&](int t, auto wrap) {
        NbrPack q;
#pragma unroll
        for (int b = 0; b < GC; ++b) q.w[b] = fetch_block16(t, b, wrap);
        return q;
    };
    auto fetch_val16 = [&](int t, auto wrap) {                      // (.col stays unset: the pipelined form keeps it in a NbrPack)
        SlotAdj p;
#pragma unroll
        for (int g = 0; g < G; ++g) p.val[g] = fetch_block16(t, GC + g, wrap);
        if constexpr (RW < D) p.lin = p.val[G - 1][3];
        else p.lin = __builtin_amdgcn_raw_buffer_load_b32(rs_lin, lane * 4, slot_of(t, wrap) * 256, 0);
        return p;
    };
    uint32_t m16 = 0xffffu;
    asm("" : "+s"(m16));                                            // (the mask in a scalar register, not a literal per instruction)
    auto unpack16 = [&](const u32x4 *w, int e) -> uint32_t {       // LDS address of entry e
        const uint32_t pw = w[e / 8][(e / 2) & 3];
        return (e & 1) ? pw >> 16 : (pw & m16);
    };
    uint32_t addr[16];                                              // N16 = 2: the addresses of the slot swept next
#ifdef MI_K2P_NOFETCH
    // TIMING-ONLY build (`make dbg`, never the shipped library; wrong chain): the adjacency of slot 0 serves every slot, so
    // the sweep loop issues no vector-memory instruction -- what the kernel would cost without its L2 traffic
    auto fetch_real = [&](int t) {
#else
    auto fetch_adj = [&](int t) {
#endif
        if constexpr (N16 != 0) {
            SlotAdj p = fetch_val16(t, no_wrap{});
            const NbrPack q = fetch_nbr16(t, no_wrap{});
#pragma unroll
            for (int b = 0; b < GC; ++b) p.col[b] = q.w[b];
            return p;
        }
        SlotAdj p;
        const int tt = t < slots ? t : slots - 1;
        const int soff = tt * SLOT_BYTES;
#pragma unroll
        for (int g = 0; g < G; ++g) {
            // (constant parts of the offset fold into the instruction's 12-bit immediate)
            const int so = soff + (g / 2) * 4096, io = (g & 1) * 2048;
            if (LW == 4 || g < G - 1) {
                p.col[g] = __builtin_amdgcn_raw_buffer_load_b128(rs_adj, lane16 + io, so, 0);
                p.val[g] = __builtin_amdgcn_raw_buffer_load_b128(rs_adj, lane16 + io + 1024, so, 0);
            } else if constexpr (LW == 3) {
                // (aligned loads only: 12-byte lanes cost the L1 more accesses than 16-byte ones) three neighbour words and
                // the lane's linear term, then two values and one
                p.col[g] = __builtin_amdgcn_raw_buffer_load_b128(rs_adj, lane16 + io, so, 0);
                const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs_adj, lane * 8 + io + 1024, so, 0);
                p.val[g] = u32x4{v.x, v.y, __builtin_amdgcn_raw_buffer_load_b32(rs_adj, lane * 4 + io + 1536, so, 0), 0u};
            } else if constexpr (LW == 2) {
                const u32x2 c = __builtin_amdgcn_raw_buffer_load_b64(rs_adj, lane * 8 + io, so, 0);
                const u32x2 v = __builtin_amdgcn_raw_buffer_load_b64(rs_adj, lane * 8 + io + 512, so, 0);
                p.col[g] = __builtin_shufflevector(c, c, 0, 1, -1, -1);
                p.val[g] = __builtin_shufflevector(v, v, 0, 1, -1, -1);
            } else {
                p.col[g][0] = __builtin_amdgcn_raw_buffer_load_b32(rs_adj, lane * 4 + io, so, 0);
                p.val[g][0] = __builtin_amdgcn_raw_buffer_load_b32(rs_adj, lane * 4 + io + 256, so, 0);
            }
        }
        if constexpr (LW == 3) p.lin = p.col[G - 1][3];            // (the trimmed packing carries it)
        else p.lin = __builtin_amdgcn_raw_buffer_load_b32(rs_lin, lane * 4, tt * 256, 0);
        return p;
    };
#ifdef MI_K2P_NOFETCH
    const SlotAdj adj0 = fetch_real(0);
    auto fetch_adj = [&](int) { return adj0; };
#endif

#ifdef MI_K2P_PROFILE
    unsigned long long tick_ = __builtin_amdgcn_s_memtime(), t_top = 0, t_gather = 0, t_sum = 0, t_rounds = 0, t_barrier = 0;
#endif
#ifndef MI_K2P_DBG_NOPRIO
    if constexpr (TW) __builtin_amdgcn_s_setprio(3);
#endif               // the sweeping wavefront is the critical path of its workgroup
    // PR ("priority rotation", round 7; the N16 = 2 forms): a SIMD holds two sweeping wavefronts.  Measured with both at 3 for
    // the whole launch (the -DMI_K2P_DBG_WAVETIMES build on the benchmark's shape): on every one of the 1024 SIMDs the one
    // that started first is the quicker, by 19 % in the median, and the launch ends with the slower ones.  So each sets its
    // priority once per sweep to 3 or 2 (the threshold wavefronts stay at 0): bit 1 of its hardware wave slot, flipped
    // every sweep.  The sweeping wavefronts of a SIMD were found in slots 1 and 3 or 0 and 2, which differ in that bit, so
    // they take the higher priority in turn; two whose slots agree in bit 1 would change together and keep the order they
    // had.  With it the median ratio is 9 % -- the older one is still the quicker everywhere, the sharing is more even, not
    // even.  s counts the sweeps of THIS launch: the chain's own counter (sw) is not involved, and no value any wavefront
    // computes depends on the priority.
    // (`make dbg DBG_FLAGS=-DMI_K2P_NO_PRIO_ROTATE`: the fixed priority, for the A/B.  The other policies measured in
    // round 7 -- the bit moving with the sweep, bit 0, the slot's parity, a lower priority across the field sums, a start
    // delay -- are in profiles/r07_k2p_simd_sharing.txt)
#if defined(MI_K2P_NO_PRIO_ROTATE) || defined(MI_K2P_DBG_NOPRIO)
    constexpr bool PR = false;
#else
    constexpr bool PR = N16 == 2;
#endif
    // HW_REG_HW_ID (register 4, all 32 bits): the wave slot of the SIMD in bits 3:0
    const uint32_t wave_slot = PR ? (__builtin_amdgcn_s_getreg(4 | (31 << 11)) & 15u) : 0u;
    auto sweep_priority = [&](int s) {
        if constexpr (PR) {
            if ((((wave_slot >> 1) ^ (uint32_t)s) & 1u) != 0u) __builtin_amdgcn_s_setprio(3);   // (the instruction takes an immediate)
            else __builtin_amdgcn_s_setprio(2);
        }
    };
#ifdef MI_K2P_DBG_WAVETIMES
    // TIMING-ONLY build (wrong states): HW_ID, XCC_ID (register 20) and the ticks around the sweeps, written over the
    // first 24 bytes of the replica-A row of states after the epilogue (scripts/k2p_wave_times.py reads them)
    const unsigned long long wt_id = (unsigned long long)__builtin_amdgcn_s_getreg(4 | (31 << 11)) |
                                     ((unsigned long long)__builtin_amdgcn_s_getreg(20 | (31 << 11)) << 32);
    const unsigned long long wt_t0 = __builtin_amdgcn_s_memtime();
#endif
    unsigned long long accepted = 0;
    uint32_t accA = 0, accB = 0;                                    // accepted moves of the running sweep, per replica
    uint32_t wa[4] = {0u, 0u, 0u, 0u}, wb[4] = {0u, 0u, 0u, 0u};
    float TA = 1.0f, TB = 1.0f;
    const float cp = a.c_pair;
    uint32_t ring_buf = 0u;                                         // TW: which half of the ring holds the group being swept

    // one slot for both replicas; `wordA` / `wordB` = this slot's random words.
    // Order of a slot: (1) the LDS reads are ISSUED -- the lane's own cell and the 16 neighbour cells; (2) while they are in
    // flight the two thresholds are computed (neglog_u2: the fp32 steps as packed instructions, one for both replicas);
    // (3) one wait; (4) the field sums; (5) the accept masks.  The reads are inline asm (hipcc adds the zero base of the
    // dynamic LDS block to every address it computes itself), so the compiler does not count them: every register they
    // write, and the thresholds, pass THROUGH the wait statement ("+v"), which makes "used only after the wait" a
    // data dependence, not a scheduling accident -- and the wait is lgkmcnt(0), so whatever LDS or scalar-memory
    // operation the compiler may place before it is waited for as well (scripts/check_asm_lds.py checks the emitted
    // code for a read of such a register ahead of its wait at build time).
    // N16 = 2: `nxt` = the packed neighbour dwords of slot t + 1 (fetched a slot ago); addr[] holds slot t's on entry, slot t + 1's on exit
    // GR: the lane's own cells and the thresholds of the group's four slots, read at the top of the group (group_reads) --
    // a lane's own cell is written by that lane in that cell's slot only, and the threshold wavefront wrote the whole group
    // before the barrier: four LDS instructions and one address a group instead of eight and eight.  They are inline asm
    // as the gathers are: slot 0's counted wait names all of them (4 + NK0 reads are in flight there, NK0 <= 15 outstanding
    // means the four are back), the later slots need no wait for them.
    // (own[h] = the cells of slots 4 g + 2 h and 4 g + 2 h + 1, in the register pair the read wrote: a copy made before the
    // wait would read the pair too early)
    struct GroupPre { u32x2 own[2]; f32x4 thr[2]; };
    auto group_reads = [&](int t, GroupPre &gp) {
        const uint32_t rb = ring_lane + ring_buf;
        asm volatile("ds_read_b128 %0, %1" : "=v"(gp.thr[0]) : "v"(rb));
        asm volatile("ds_read_b128 %0, %1 offset:1024" : "=v"(gp.thr[1]) : "v"(rb));
        // own cells 256 bytes apart: one address.  The last group of a sweep of 4 g + 1 .. 4 g + 3 slots (wave-uniform): the
        // ring lies behind the cells and is not read as one -- a slot that does not exist reads its neighbour's cell again
        const uint32_t cb = (uint32_t)(t * 256 + lane * 4);
        if (t + 1 < slots) asm volatile("ds_read2st64_b32 %0, %1 offset1:1" : "=v"(gp.own[0]) : "v"(cb));
        else asm volatile("ds_read2st64_b32 %0, %1" : "=v"(gp.own[0]) : "v"(cb));
        if (t + 3 < slots) asm volatile("ds_read2st64_b32 %0, %1 offset0:2 offset1:3" : "=v"(gp.own[1]) : "v"(cb));
        else asm volatile("ds_read2st64_b32 %0, %1" : "=v"(gp.own[1]) : "v"((t + 2 < slots ? t + 2 : slots - 1) * 256 + lane * 4));
    };
    auto slot_body = [&](auto c_in_group, int t, const SlotAdj &cur, NbrPack &nxt, uint32_t wordA, uint32_t wordB, GroupPre &gp) {
        constexpr int C = decltype(c_in_group)::value;
        const int i = t * 64 + lane;
        uint32_t own;                                               // [x_A | x_B] of this lane's variable
        float gA = __uint_as_float(cur.lin), gB = gA;               // (lanes past n carry lin = +inf: never accepted)
        float thrA = 0.0f, thrB = 0.0f;
        f32x2_t thr2 = {0.0f, 0.0f};
        // what the accept masks need of the lane's OWN cell (TW: computed under the gathers, see below)
        uint32_t xiA = 0u, xiB = 0u, sgA = 0u, sgB = 0u;
        uint64_t XA = 0ull, XB = 0ull;
        f32x2_t cs = {0.0f, 0.0f}, csf = {0.0f, 0.0f};
        int ownA = 0, ownB = 0;
        auto own_terms = [&]() {
            xiA = (own >> 13) & 1u;                                 // 0x3c00 -> 1
            xiB = own >> 29;
            XA = __ballot((own & 0xffffu) != 0u);
            XB = __ballot((own >> 16) != 0u);
            sgA = xiA << 31;                                        // dE = x ? -f : f
            sgB = xiB << 31;
            cs = f32x2_t{__uint_as_float(__float_as_uint(cp) ^ sgA), __uint_as_float(__float_as_uint(cp) ^ sgB)};
            ownA = SA - (int)xiA;
            ownB = SB - (int)xiB;
            csf = cs * f32x2_t{(float)ownA, (float)ownB};           // the oracle's c * (float)(s - x): one packed multiply
        };
        K2P_TICK(t_top);
#pragma unroll
        for (int g0 = 0; g0 < G; g0 += 4) {
            constexpr int NK0 = RW < 16 ? RW : 16;                  // gathers of the first block of four groups
            const int NK = g0 == 0 ? NK0 : (RW - 4 * g0 < 16 ? RW - 4 * g0 : 16);
            uint32_t word[16];                                      // (words past NK are never read nor written)
            // the packed neighbour word IS the LDS byte address of its cell (one wavefront per workgroup, no static LDS)
            if (g0 == 0 && !GR) asm volatile("ds_read_b32 %0, %1" : "=v"(own) : "v"(i * 4));
            // (TW: the ring read second, so that "at most 15 reads outstanding" below means the own cell and the thresholds are back)
            if (g0 == 0 && TW && !GR) asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(thr2) : "v"(ring_lane + ring_buf), "n"(C * 512));
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k < NK)
#ifdef MI_K2P_DBG_LINEAR   /* timing only: conflict-free addresses */
                asm volatile("ds_read_b32 %0, %1" : "=v"(word[k]) : "v"((cur.col[g0 + k / 4][k & 3] & 0x3f00u) + lane * 4));
#else
                {
                    if constexpr (N16 == 2) asm volatile("ds_read_b32 %0, %1" : "=v"(word[k]) : "v"(addr[k]));
                    else if constexpr (N16 == 1) asm volatile("ds_read_b32 %0, %1" : "=v"(word[k]) : "v"(unpack16(cur.col, 4 * g0 + k)));
                    else
                asm volatile("ds_read_b32 %0, %1" : "=v"(word[k]) : "v"(cur.col[g0 + k / 4][k & 3]));
                }
#endif
            if (g0 == 0 && TW) {
                // NK0 + 2 LDS reads are in flight and they return in order: with at most NK0 (15 at most: the counter's
                // width) outstanding the lane's own cell and the thresholds are here -- everything that depends only on
                // them is computed UNDER the gathers (the second wait names its results, so it cannot sink below it)
                // (N16 = 2: the next slot's neighbour dwords pass through this wait, so their unpack cannot rise above the gathers)
                if constexpr (GR) {
                    // (slot 0: the group's reads are the oldest in flight.  Slots 1 to 3: nothing to wait for; the empty
                    // statement keeps the own-cell terms and the unpack below the gathers' issue as the wait does)
                    if constexpr (C == 0)
                        asm volatile("s_waitcnt lgkmcnt(%6)"
                                     : "+v"(gp.own[0]), "+v"(gp.own[1]), "+v"(gp.thr[0]), "+v"(gp.thr[1]), "+v"(nxt.w[0]), "+v"(nxt.w[1])
                                     : "n"(NK0 < 15 ? NK0 : 15) : "memory");
                    else
                        asm volatile("" : "+v"(gp.own[C >> 1]), "+v"(gp.thr[C >> 1]), "+v"(nxt.w[0]), "+v"(nxt.w[1]));
                    own = gp.own[C >> 1][C & 1];
                    thr2 = f32x2_t{gp.thr[C >> 1][2 * (C & 1)], gp.thr[C >> 1][2 * (C & 1) + 1]};
                } else if constexpr (N16 == 2)
                    asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(own), "+v"(thr2), "+v"(nxt.w[0]), "+v"(nxt.w[1]) : "n"(NK0 < 15 ? NK0 : 15) : "memory");
                else
                asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(own), "+v"(thr2) : "n"(NK0 < 15 ? NK0 : 15) : "memory");
#ifndef MI_K2P_DBG_TERMS_AFTER   /* (timing only: the terms after the full wait, as before) */
                own_terms();
#endif
                if constexpr (N16 == 2) {
                    // ... and into the registers the gathers above have consumed; the empty statements tie each result to
                    // this side of the full wait (volatile statements keep their order)
#pragma unroll
                    for (int k = 0; k < NK0; ++k) {
                        addr[k] = unpack16(nxt.w, k);
                        asm volatile("" : "+v"(addr[k]));
                    }
                }
                asm volatile("s_waitcnt lgkmcnt(0)"
                             : "+v"(word[0]), "+v"(word[1]), "+v"(word[2]), "+v"(word[3]), "+v"(word[4]), "+v"(word[5]),
                               "+v"(word[6]), "+v"(word[7]), "+v"(word[8]), "+v"(word[9]), "+v"(word[10]), "+v"(word[11]),
                               "+v"(word[12]), "+v"(word[13]), "+v"(word[14]), "+v"(word[15]), "+v"(csf)
                             :: "memory");
                thrA = thr2.x;
                thrB = thr2.y;
            } else if (g0 == 0) {
                asm volatile("" : "+v"(wordA), "+v"(wordB));        // (keeps the threshold arithmetic behind the reads' issue)
                const f32x2_t thr = neglog_u2(wordA, wordB) * f32x2_t{TA, TB};
                thrA = thr.x;
                thrB = thr.y;
                asm volatile("s_waitcnt lgkmcnt(0)"
                             : "+v"(word[0]), "+v"(word[1]), "+v"(word[2]), "+v"(word[3]), "+v"(word[4]), "+v"(word[5]),
                               "+v"(word[6]), "+v"(word[7]), "+v"(word[8]), "+v"(word[9]), "+v"(word[10]), "+v"(word[11]),
                               "+v"(word[12]), "+v"(word[13]), "+v"(word[14]), "+v"(word[15]), "+v"(own), "+v"(thrA), "+v"(thrB)
                             :: "memory");
            } else {
                asm volatile("s_waitcnt lgkmcnt(0)"
                             : "+v"(word[0]), "+v"(word[1]), "+v"(word[2]), "+v"(word[3]), "+v"(word[4]), "+v"(word[5]),
                               "+v"(word[6]), "+v"(word[7]), "+v"(word[8]), "+v"(word[9]), "+v"(word[10]), "+v"(word[11]),
                               "+v"(word[12]), "+v"(word[13]), "+v"(word[14]), "+v"(word[15])
                             :: "memory");
            }
            K2P_TICK(t_gather);
#pragma unroll
            for (int k = 0; k < NK; ++k) {
                const float v = __uint_as_float(cur.val[g0 + k / 4][k & 3]);
                gA = __builtin_fmaf(v, half_lo(word[k]), gA);       // fma(val, x, g): the oracle's conditional add
                gB = __builtin_fmaf(v, half_hi(word[k]), gB);
            }
        }
#ifdef MI_K2P_DBG_TERMS_AFTER
        own_terms();
#else
        if constexpr (!TW) own_terms();
#endif
        if (WGT && t == wslot) {
            // ---- the slot of the weighted variables: a serial sweep per replica (few lanes, no sparse couplings) ----
            const uint64_t FA = weighted_slot_sweep(gA, thrA, wl, cp, xiA, SA, lane);
            const uint64_t FB = weighted_slot_sweep(gB, thrB, wl, cp, xiB, SB, lane);
            accA += (uint32_t)__popcll(FA);
            accB += (uint32_t)__popcll(FB);
            uint32_t fA, fB;
            asm("v_cndmask_b32 %0, 0, %1, %2" : "=v"(fA) : "v"(0x3c00u), "s"(FA));
            asm("v_cndmask_b32 %0, 0, %1, %2" : "=v"(fB) : "v"(0x3c000000u), "s"(FB));
            cell[i] = own ^ fA ^ fB;
            K2P_TICK(t_rounds);
            return;
        }
        const f32x2_t gs = {__uint_as_float(__float_as_uint(gA) ^ sgA), __uint_as_float(__float_as_uint(gB) ^ sgB)};
        // accept masks by fixed-point rounds (see k_anneal_csr_rank1): both replicas advance together; the oracle's
        // g + c * (float)(s - x) as one packed multiply and one packed add (no contraction)
        f32x2_t de = gs + csf;
        bool mA = de.x < thrA, mB = de.y < thrB;
        uint64_t AA = __ballot(mA), AB = __ballot(mB);
        K2P_TICK(t_sum);
        if ((AA | AB) != 0ull) {                                    // wave-uniform
            const int baseA = ownA - (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(XA >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)XA, 0u));
            const int baseB = ownB - (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(XB >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)XB, 0u));
            // (the loop ends by itself: a lane's decision depends on the masks of the lanes below it only, so after k rounds the
            // lowest k lanes are final whatever the data -- NaNs included, a compare with one is just false -- and round 65
            // repeats round 64.  Everything that leaves the loop is a wave-uniform mask: a per-lane flag live across it costs
            // six scalar instructions a round, a round counter five)
            uint64_t BA = AA ^ XA, BB = AB ^ XB;                    // the states after the moves guessed so far
#ifndef MI_K2P_DBG_NOROUNDS   /* (timing only: the first masks stand) */
#pragma nounroll
            for (;;) {
                const int sA = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(BA >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)BA, (uint32_t)baseA));
                const int sB = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(BB >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)BB, (uint32_t)baseB));
                de = gs + cs * f32x2_t{(float)sA, (float)sB};
                const uint64_t NBA = __ballot(de.x < thrA) ^ XA, NBB = __ballot(de.y < thrB) ^ XB;
                uint64_t d0 = NBA ^ BA, d1 = NBB ^ BB;
                asm("" : "+s"(d0), "+s"(d1));                       // (opaque: hipcc turns (a^b)|(c^d) == 0 into two compares and selects)
                BA = NBA;
                BB = NBB;
                if ((d0 | d1) == 0ull) break;
            }
#endif
            AA = BA ^ XA;
            AB = BB ^ XB;
            // sum(x) moves by popc(new states) - popc(old states) of the slot
            SA += __popcll(BA) - __popcll(XA);
            SB += __popcll(BB) - __popcll(XB);
            accA += (uint32_t)__popcll(AA);
            accB += (uint32_t)__popcll(AB);
            // toggling a state is one XOR of its half; every lane stores its cell (unchanged cells keep their word)
            uint32_t tA, tB;
            asm("v_cndmask_b32 %0, 0, %1, %2" : "=v"(tA) : "v"(0x3c00u), "s"(AA));
            asm("v_cndmask_b32 %0, 0, %1, %2" : "=v"(tB) : "v"(0x3c000000u), "s"(AB));
            cell[i] = own ^ tA ^ tB;
        }
        K2P_TICK(t_rounds);
    };

    // N16 = 2: the values one slot ahead (cP / cQ), the neighbour dwords TWO (cNA / cNB), the unpacked addresses of one slot.
    // At the top of a group of four at slot t: cP = values of t, cNA = neighbour dwords of t + 1, addr[] = addresses of t.
    // CY: the prefetch index wraps (slot_of), so a sweep ends with exactly that for slot 0 of the next one and only the first
    // sweep of a launch fills the pipeline (the last one fetches slots 0 and 1 for nothing) -- a sweep of 4 g + 1 or 4 g + 3
    // slots ends with it in cQ / cNB and moves it over.  (One loop per kernel: both loops in one cost 40 registers.)
    SlotAdj cP, cQ;
    NbrPack cNA, cNB;
    GroupPre gp;
    auto sweep16 = [&]() {
        constexpr bool W = CY;
        const integral_constant<bool, CY> wrap;
#pragma unroll 1
        for (int t = 0; t < slots; t += 4) {
            K2P_TICK(t_top);
            __builtin_amdgcn_s_barrier();                           // this group's thresholds are in the ring
            K2P_TICK(t_barrier);
            if constexpr (GR) group_reads(t, gp);
            cQ = fetch_val16(t + 1, wrap);
            cNB = fetch_nbr16(t + 2, wrap);
            slot_body(integral_constant<int, 0>{}, t, cP, cNA, wa[0], wb[0], gp);
            if (t + 1 < slots) {                                    // wave-uniform
                cP = fetch_val16(t + 2, wrap);
                cNA = fetch_nbr16(t + 3, wrap);
                slot_body(integral_constant<int, 1>{}, t + 1, cQ, cNB, wa[1], wb[1], gp);
                if (t + 2 < slots) {
                    cQ = fetch_val16(t + 3, wrap);
                    cNB = fetch_nbr16(t + 4, wrap);
                    slot_body(integral_constant<int, 2>{}, t + 2, cP, cNA, wa[2], wb[2], gp);
                    if (!W || t + 3 < slots) {
                        cP = fetch_val16(t + 4, wrap);
                        cNA = fetch_nbr16(t + 5, wrap);
                        if (t + 3 < slots) slot_body(integral_constant<int, 3>{}, t + 3, cQ, cNB, wa[3], wb[3], gp);
                    } else {
                        cP = cQ;
                        cNA = cNB;
                    }
                }
            } else if (W) {
                cP = cQ;
                cNA = cNB;
            }
            ring_buf ^= 2048u;
        }
    };
    for (int s = 0; s < a.num_sweeps; ++s) {
        if constexpr (!TW) {
            if (a.temps_per_replica) {
                TA = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.temps[rA])));
                TB = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.temps[liveB ? rB : rA])));
            } else {
                TA = TB = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(a.temps[s])));
            }
        }
        const uint32_t sw = (uint32_t)s + a.sweep_offset;
        sweep_priority(s);
        if constexpr (N16 == 2) {
            if (!CY || s == 0) {
                cP = fetch_val16(0, no_wrap{});
                cNA = fetch_nbr16(0, no_wrap{});
#pragma unroll
                for (int k = 0; k < (RW < 16 ? RW : 16); ++k) addr[k] = unpack16(cNA.w, k);
                cNA = fetch_nbr16(1, no_wrap{});
            }
            sweep16();
        } else {
            NbrPack none;
            // four slots per trip (one Philox block per replica), the adjacency one slot ahead in two register sets
            SlotAdj P = fetch_adj(0), Q;
    #pragma unroll 1
            for (int t = 0; t < slots; t += 4) {
                if constexpr (TW) {
                    K2P_TICK(t_top);
                    __builtin_amdgcn_s_barrier();                       // this group's thresholds are in the ring
                    K2P_TICK(t_barrier);
                } else {
                    philox4x32_10((uint32_t)((t >> 2) * 64 + lane), sw, gidA, 0u, a.seed_lo, a.seed_hi, wa);
                    philox4x32_10((uint32_t)((t >> 2) * 64 + lane), sw, gidB, 0u, a.seed_lo, a.seed_hi, wb);
                }
                Q = fetch_adj(t + 1);
                slot_body(integral_constant<int, 0>{}, t, P, none, wa[0], wb[0], gp);
                if (t + 1 < slots) {                                    // wave-uniform
                    P = fetch_adj(t + 2);
                    slot_body(integral_constant<int, 1>{}, t + 1, Q, none, wa[1], wb[1], gp);
                    if (t + 2 < slots) {
                        Q = fetch_adj(t + 3);
                        slot_body(integral_constant<int, 2>{}, t + 2, P, none, wa[2], wb[2], gp);
                        P = fetch_adj(t + 4);
                        if (t + 3 < slots) slot_body(integral_constant<int, 3>{}, t + 3, Q, none, wa[3], wb[3], gp);
                    }
                }
                if constexpr (TW) ring_buf ^= 2048u;
            }
        }
        accepted += (unsigned long long)accA + (liveB ? (unsigned long long)accB : 0ull);
        accA = accB = 0;
    }
#ifdef MI_K2P_DBG_WAVETIMES
    const unsigned long long wt_t1 = __builtin_amdgcn_s_memtime();
#endif

    // ---- epilogue: states out, exact fp64 energies (same sums as k_anneal_csr_rank1) ----
    // The sums and their order are the specification's; the order of the loads is not: per slot all the neighbour indices
    // and all the values are requested together, then the cells, then the additions in the order of k -- two round trips
    // per slot and replica instead of 2 D dependent ones -- and the fp64 / fp32 choice of the values is made per slot, not
    // per entry (one copy of the loop: two cost the weighted form's sweep loop a register).
    const bool has64 = a.ell_val64 != nullptr;
#pragma unroll 1
    for (int rep = 0; rep < 2; ++rep) {
        if (rep == 1 && !liveB) break;
        const int r = rep ? rB : rA;
        const int sh = rep ? 16 : 0;
        uint8_t *dst = static_cast<uint8_t *>(a.states) + (size_t)r * n;
        long long cnt = 0, cnt2 = 0;                               // sum_j w_j x_j, sum_j w_j^2 x_j
        double e = 0.0;
        for (int t = 0; t < slots; ++t) {
            const int i = t * 64 + lane;
            const bool on = ((cell[i] >> sh) & 0xffffu) != 0u;
#ifdef MI_K2P_DBG_WAVETIMES   /* (the record's bytes belong to lane 0's stores below) */
            if (rep == 0 && i < 24) { } else
#endif
            if (i < n) dst[i] = (uint8_t)on;
            if (WGT && t == wslot) {
                cnt += wave_sum_i64(on ? (long long)wl : 0ll);
                cnt2 += wave_sum_i64(on ? (long long)wl * wl : 0ll);
            } else {
                const int c1 = __popcll(__ballot(on));
                cnt += c1;
                cnt2 += c1;
            }
            if (!on) continue;
            double acc = 0.0;
#ifdef MI_K2P_NO_EPI
            for (int k = 0; k < D; ++k) {
                const size_t at = ((size_t)t * D + k) * 64 + lane;
                const uint32_t cc = a.ell_col[at];
                const double vv = a.ell_val64 ? a.ell_val64[at] : (double)a.ell_val[at];
                if (((cell[cc] >> sh) & 0xffffu) != 0u) acc += vv;
            }
#else
#pragma unroll
            for (int k0 = 0; k0 < D; k0 += 16) {
                uint32_t cc[16], cw[16];
                double vv[16];
#pragma unroll
                for (int k = 0; k < 16; ++k) cc[k] = a.ell_col[((size_t)t * D + k0 + k) * 64 + lane];
                if (has64) {
#pragma unroll
                    for (int k = 0; k < 16; ++k) vv[k] = a.ell_val64[((size_t)t * D + k0 + k) * 64 + lane];
                } else {
#pragma unroll
                    for (int k = 0; k < 16; ++k) vv[k] = (double)a.ell_val[((size_t)t * D + k0 + k) * 64 + lane];
                }
#pragma unroll
                for (int k = 0; k < 16; ++k) cw[k] = cell[cc[k]];
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if (((cw[k] >> sh) & 0xffffu) != 0u) acc += vv[k];
            }
#endif
            e += (a.lin64 ? a.lin64[i] : (double)a.lin[i]) + 0.5 * acc;
        }
        e = wave_sum_f64(e);
        if (lane == 0) a.energy[r] = binary_chain_finish(a.ell_val64, a.c_pair, a.c_pair64, a.offset, e, cnt, cnt2);
    }
    if (lane == 0) atomicAdd(&a.stats[1], accepted);
#ifdef MI_K2P_DBG_WAVETIMES
    if (lane == 0 && n >= 24 && ((size_t)rA * n) % 4 == 0) {        // (rows of 64 k bytes: the padded layouts)
        uint32_t *q = reinterpret_cast<uint32_t *>(static_cast<uint8_t *>(a.states) + (size_t)rA * n);
        q[0] = (uint32_t)wt_id; q[1] = (uint32_t)(wt_id >> 32);
        q[2] = (uint32_t)wt_t0; q[3] = (uint32_t)(wt_t0 >> 32);
        q[4] = (uint32_t)wt_t1; q[5] = (uint32_t)(wt_t1 >> 32);
    }
#endif
#ifdef MI_K2P_PROFILE
    if (lane == 0) {
        atomicAdd(&a.stats[8], t_top); atomicAdd(&a.stats[9], t_gather); atomicAdd(&a.stats[10], t_sum);
        atomicAdd(&a.stats[11], t_rounds); atomicAdd(&a.stats[12], t_barrier);
    }
#endif
}

}  // namespace

// a.adj4 holds the packing the plan names (plan_k2p, csrc/mi_sa_plan.h)
int mi_launch_csr_rank1_pair(const EllArgs &a, const AnnealPlan &plan, hipStream_t st)
{
    if (!a.adj4) return fail(MI_EHIP, "csr_rank1 pair kernel: packed adjacency missing");
#ifdef MI_K2P_NOFETCH
    if (plan.nbr16) return fail(MI_EUNSUPPORTED, "the timing builds are arms of the 32-bit packing: set k2_nbr16 = 2");
#endif
    const int rw = plan.trim_rw ? plan.trim_rw : plan.D;
    // the pipelined form carries its prefetch over the sweep boundary where a sweep is longer than the prefetch is deep
#ifdef MI_K2P_NO_CARRY
    const bool carry = false;
#else
    const bool carry = a.slots >= 6;
#endif
#define MI_K2P(D_, TW_, WGT_, RW_, N16_) \
    if (plan.D == D_ && plan.tw == TW_ && plan.weighted == WGT_ && rw == RW_ && (plan.nbr16 ? N16_ != 0 : N16_ == 0)) { \
        if (N16_ == 2 && carry) return launch_planned(k_anneal_csr_rank1_pair<D_, TW_, WGT_, RW_, N16_, N16_ == 2>, a, plan, st); \
        return launch_planned(k_anneal_csr_rank1_pair<D_, TW_, WGT_, RW_, N16_>, a, plan, st); \
    }
    MI_K2P(16, true, true, 16, 0) MI_K2P(16, false, true, 16, 0)                          // pair-term weights
    MI_K2P(16, true, false, 15, 2) MI_K2P(16, true, false, 14, 2) MI_K2P(16, true, false, 13, 2)   // trimmed rows, 16-bit neighbour words
    MI_K2P(16, true, false, 15, 0) MI_K2P(16, true, false, 14, 0) MI_K2P(16, true, false, 13, 0)   // trimmed rows
    MI_K2P(16, true, false, 16, 2) MI_K2P(32, false, false, 32, 1)                        // full rows, 16-bit neighbour words
    MI_K2P(16, true, false, 16, 0) MI_K2P(16, false, false, 16, 0) MI_K2P(32, false, false, 32, 0)
#undef MI_K2P
    return fail(MI_EUNSUPPORTED, "csr_rank1 pair kernel: slot-ELL width %d not built", a.D);
}

}  // namespace mi_sa_impl
