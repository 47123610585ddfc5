// mi_sa_plan.h -- which anneal kernel serves a structured model (MI_KIND_CSR_RANK1: K2, K2p, K2w, K2s; MI_KIND_POTTS_CSR:
// K3, K3f), decided in ONE place and in plain host code: no HIP header or type, so this file compiles with any C++17
// compiler and is tested without a GPU (mi_sa_plan_anneal, tests/test_anneal_plan.py, tests/host/plan_pack_main.cpp).
//
//   slot_model_facts   what a model is eligible for (computed once, when the model is created)
//   plan_csr_rank1 /   the kernel of one anneal call: family, template coordinates, packing, LDS, grid.  The launchers
//   plan_potts         (mi_launch_* in the kernel files) are switches from these coordinates to an instantiation.
//   plan_kernel_name   the string mi_sa_last_kernel_name reports for a plan
#pragma once

#include <climits>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/mi_sa.h"

namespace mi_sa_plan {

constexpr size_t kLdsBytes = 160 * 1024;     // LDS of one CU
// K2s's LDS behind the cells (csrc/sparse_split_kernels.hip)
constexpr int kCommBytes = 8 * 16;               // eight exchange slots of four ints (the waves' net changes)
constexpr int kRingBytes = 4 * 64 * 16;          // NW > 1: four groups of random words in flight, [4][64 lanes][4 words]

inline int plan_fail(std::string *err, int code, const char *fmt, ...) __attribute__((format(printf, 3, 4)));
inline int plan_fail(std::string *err, int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (err) *err = buf;
    return code;
}

// ------------------------------------------------------------------------------------------------
// the model
// ------------------------------------------------------------------------------------------------
struct SlotModelFacts {
    int kind = 0, n = 0, slots = 0, K = 0, max_degree = 0;
    int D = 0;                       // slot-ELL width: 16 / 32 / 64, else the next multiple of 16 (the runtime-width kernels)
    int state_bytes = 2;             // K2's state in LDS: a half (2), a byte (1) or a bit (0) per variable
    bool any_in_slot_edge = false;   // some edge joins two seats of one 64-seat slot
    int free_block = 0;              // binary models: widest block of seats (256 / 128 / 64; 0 = none) that holds no edge anywhere
    bool has_pair_packing = false;   // K2p / K2w / K2s: the packing with neighbour word = 4 * index
    bool has_pair16 = false;         // ... and K2p's with 16-bit neighbour words
    int trim_rw = 0;                 // ... and K2p's trimmed ones: every row has at most this many (13..15) entries at D = 16; 0 = none
    bool has_fast_packing = false;   // K3f: the packing with neighbour word = 2 * index
};

// The size limits of the two structured kinds (checked before anything is allocated).
inline int slot_model_size_check(int kind, int n, int K, std::string *err)
{
    if (n < 1) return plan_fail(err, MI_EINVAL, "n must be >= 1 (got %d)", n);
    if (kind == MI_KIND_CSR_RANK1 && n > (1 << 20))
        return plan_fail(err, MI_EUNSUPPORTED, "csr_rank1 kernel supports n <= 1048576 (got %d)", n);
    if (kind == MI_KIND_POTTS_CSR && (K < 1 || K > 64))
        return plan_fail(err, MI_EUNSUPPORTED, "potts kernel supports 1 <= K <= 64 cases (got %d)", K);
    if (kind == MI_KIND_POTTS_CSR && n > 40000)
        return plan_fail(err, MI_EUNSUPPORTED, "potts kernel supports n <= 40000 (got %d)", n);
    return MI_OK;
}

// CSR (both directions stored) -> what the model is eligible for.  forced_state: the value of MI_K2_STATE (bit | byte |
// half, nullable), which narrows K2's state width: A/B timing of the three forms on one model.
inline int slot_model_facts(int kind, const int32_t *rowptr, const int32_t *col, int n, int K, const char *forced_state,
                            SlotModelFacts *out, std::string *err)
{
    SlotModelFacts f;
    f.kind = kind; f.n = n; f.K = K;
    for (int i = 0; i < n; ++i) {
        const int d = rowptr[i + 1] - rowptr[i];
        if (d < 0) return plan_fail(err, MI_EINVAL, "rowptr is not monotone at %d", i);
        if (d > f.max_degree) f.max_degree = d;
    }
    // rows up to 64 wide are register resident in K2 and K3; wider ones (any multiple of 16 up to 4096) run on the
    // runtime-width forms of the same kernels, which read the adjacency from L2 inside the field sum
    if (f.max_degree > 4096)
        return plan_fail(err, MI_EUNSUPPORTED, "max degree %d exceeds the widest adjacency layout (4096); use the dense kernel", f.max_degree);
    const int maxdeg = f.max_degree;
    f.D = maxdeg <= 16 ? 16 : (maxdeg <= 32 ? 32 : (maxdeg <= 64 ? 64 : ((maxdeg + 15) / 16) * 16));
    f.slots = (n + 63) / 64;
    for (int i = 0; i < n; ++i)
        for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) {
            if (col[e] < 0 || col[e] >= n || col[e] == i) return plan_fail(err, MI_EINVAL, "bad column %d in row %d", col[e], i);
            if ((col[e] >> 6) == (i >> 6)) f.any_in_slot_edge = true;
        }
    const size_t slots = (size_t)f.slots;
    if (kind == MI_KIND_POTTS_CSR) {
        // K3f (csrc/potts_fast_kernels.hip): every slot free of internal edges, 2 bytes of LDS per seat + the cluster sizes
        f.has_fast_packing = !f.any_in_slot_edge && (f.D == 16 || f.D == 32) && slots * 128 + 256 <= kLdsBytes;
    } else if (kind == MI_KIND_CSR_RANK1) {
        // state in LDS: a half per variable while 16 replicas fit one CU (n <= 4608), else a byte (n <= 9216), else a bit
        const bool fits_half = slots * 128 * 16 <= 144 * 1024, fits_byte = slots * 64 * 16 <= 144 * 1024;
        f.state_bytes = fits_half ? 2 : (fits_byte ? 1 : 0);
        if (forced_state && !strcmp(forced_state, "byte") && fits_byte) f.state_bytes = 1;
        if (forced_state && !strcmp(forced_state, "bit")) f.state_bytes = 0;
        // K2s / K2w: the widest block of whole slots that holds no edge (a layout planned with slot = 128 / 256 seats)
        f.free_block = f.any_in_slot_edge ? 0 : 64;
        for (int B : {256, 128}) {
            if (f.any_in_slot_edge || f.slots % 4 != 0) continue;    // (whole groups of four slots: one Philox block each)
            bool ok = true;
            for (int i = 0; i < n && ok; ++i)
                for (int e = rowptr[i]; e < rowptr[i + 1]; ++e)
                    if (col[e] / B == i / B) { ok = false; break; }
            if (ok) { f.free_block = B; break; }
        }
        // K2p: every slot free of internal edges, D = 16 / 32, 4 bytes per variable (+ the ring of thresholds) fit a CU's LDS
        // (the pair packing serves K2p and the few-replica kernels: 4 bytes of LDS per seat and replica pair / replica;
        // whether a RUN fits the CUs' LDS is decided per anneal, plan_csr_rank1)
        f.has_pair_packing = !f.any_in_slot_edge && (f.D == 16 || f.D == 32) && slots * 256 + 4096 <= kLdsBytes;
        f.has_pair16 = f.has_pair_packing && f.slots <= 256;         // (LDS byte addresses 4 j of 16 bits)
        // entries maxdeg .. 15 are padding in every row: K2p's trimmed form neither fetches nor gathers them
        if (f.has_pair_packing && f.D == 16 && maxdeg >= 13 && maxdeg < 16) f.trim_rw = maxdeg;
    }
    *out = f;
    return MI_OK;
}

// ------------------------------------------------------------------------------------------------
// the run and the options
// ------------------------------------------------------------------------------------------------
struct RunFacts {
    int R = 1;
    int cus = 0;                     // compute units of the device (0: 256)
    int pair_weight_slot = -1;       // binary models: the slot with pair-term weights other than 1 (-1: none)
    bool node_weights = false;       // Potts: node weights of the pair term (chain 2d)
    int min_cluster_size = 0;        // Potts: hard lower bound on every cluster's size
};

struct PlanOptions {
    int k2_waves = 0;                // (99: K3 keeps its serial move loop -- A/B timing)
    int k2_pair = 0;                 // K2p: 0 auto (runs of more replicas than the chip has SIMDs), 1 always when eligible, 2 never
    int k2_split = 0;                // K2s (csrc/sparse_split_kernels.hip): 0 auto (few replicas: its one-wavefront form), 1 always when eligible (2 / 4 wavefronts per replica on models laid out in blocks of 128 / 256 seats), 2 never
    int k2_split_max = 1024;         // ... auto: runs of up to this many replicas (a wavefront per SIMD at most)
    int k2_wide = 0;                 // models laid out in blocks of 128 / 256 seats, few replicas: 0 / 1 one wavefront sweeps a block per step (K2w), 2 a workgroup of 2 / 4 wavefronts does (K2s)
    int k2_tw = 0;                   // a threshold wavefront per workgroup: 0 auto (when built for the width), 1 on, 2 off
    int k2_trim = 0;                 // K2p's trimmed rows (rows of 13..15 entries at D = 16): 0 auto / 1 on (when built), 2 off
    int k2_nbr16 = 0;                // K2p's 16-bit neighbour words: 0 auto / 1 on (wherever built), 2 off (the 32-bit packings)
    int k3_fast = 0;                 // K3f (csrc/potts_fast_kernels.hip): 0 auto (when the model is eligible), 2 never
};

// every key of mi_sa_set_option that the planner reads, with the values it takes ([lo, hi], or `also`)
struct PlanOptionKey { const char *key; int PlanOptions::*field; long lo, hi, also; };
inline constexpr PlanOptionKey kPlanOptionKeys[] = {
    {"k2_waves", &PlanOptions::k2_waves, 0, 16, 99},
    {"k2_pair", &PlanOptions::k2_pair, 0, 2, -1},
    {"k2_split", &PlanOptions::k2_split, 0, 2, -1},
    {"k2_split_max", &PlanOptions::k2_split_max, 0, LONG_MAX, -1},
    {"k2_wide", &PlanOptions::k2_wide, 0, 2, -1},
    {"k2_tw", &PlanOptions::k2_tw, 0, 2, -1},
    {"k2_trim", &PlanOptions::k2_trim, 0, 2, -1},
    {"k2_nbr16", &PlanOptions::k2_nbr16, 0, 2, -1},
    {"k3_fast", &PlanOptions::k3_fast, 0, 2, -1},
};

// true: `key` is one of the planner's options and takes `value`
inline bool plan_option_set(PlanOptions &o, const char *key, long value)
{
    for (const PlanOptionKey &k : kPlanOptionKeys)
        if (!strcmp(key, k.key) && ((value >= k.lo && value <= k.hi) || value == k.also)) {
            o.*k.field = (int)value;
            return true;
        }
    return false;
}

// ------------------------------------------------------------------------------------------------
// the plan
// ------------------------------------------------------------------------------------------------
enum PlanFamily { PLAN_K2, PLAN_K2P, PLAN_K2W, PLAN_K2S, PLAN_K3, PLAN_K3F };

// which packed adjacency EllArgs::adj4 points at
enum PlanPacking {
    PACK_STATE,          // K2: neighbour word = where the neighbour's state lives in LDS (half / byte / bit)
    PACK_PAIR,           // neighbour word = 4 * index
    PACK_PAIR_TRIM,      // ... without the entries past the longest row (pack_pair_adjacency)
    PACK_PAIR16,         // 16-bit neighbour words (pack_pair_adjacency16)
    PACK_PAIR16_TRIM,    // ... with the linear term in the sixteenth value
    PACK_FAST,           // K3f: neighbour word = 2 * index
    PACK_NONE,           // K3 reads the row-major copy
};

struct AnnealPlan {
    int family = PLAN_K2;
    // template coordinates
    int D = 0;                       // slot-ELL width; 0: the runtime-width form
    int state_bytes = 0;             // K2
    int step = 1;                    // K2w: slots per step; K2s: wavefronts per replica; K3: replicas per workgroup
    int KM = 0;                      // K3f: cluster-size registers (8 / 16)
    int trim_rw = 0;                 // K2p: entries per row of the trimmed packing (0: full rows)
    bool nbr16 = false;              // K2p: 16-bit neighbour words
    bool tw = false;                 // a threshold wavefront beside the sweeping one (same chain)
    bool weighted = false;           // pair-term weights (binary) / node weights (Potts)
    bool size_test = false;          // K3f: the kernels with the minimum-cluster-size test
    // the launch
    int packing = PACK_NONE;
    int adj_bytes = 0;               // packed adjacency bytes a wavefront fetches per slot (0: a kernel without such a packing)
    size_t lds_bytes = 0;
    int ring_off = 0;                // K2 with tw: byte offset of the ring of thresholds in LDS
    int grid = 0, block = 0;
};

inline bool ell_width_built(int D) { return D == 16 || D == 32 || D == 64 || (D > 64 && D % 16 == 0); }

// K2: one wavefront = one replica = one workgroup; the only LDS is the state (a bit, a byte or a half per variable) -- and,
// with a threshold wavefront beside the sweeping one, the ring of thresholds behind it
inline int plan_k2(const SlotModelFacts &f, const RunFacts &run, bool tw, AnnealPlan *out, std::string *err)
{
    AnnealPlan p;
    p.family = PLAN_K2; p.D = f.D <= 64 ? f.D : 0; p.state_bytes = f.state_bytes; p.packing = PACK_STATE;
    p.weighted = run.pair_weight_slot >= 0;
    // tw is built for the register-resident widths of large models: bit and byte state at D = 16 / 32
    p.tw = tw && (f.D == 16 || f.D == 32) && f.state_bytes <= 1;
    if (!ell_width_built(f.D)) return plan_fail(err, MI_EUNSUPPORTED, "slot-ELL width %d not built", f.D);
    p.lds_bytes = (size_t)f.slots * (f.state_bytes == 2 ? 128 : (f.state_bytes == 1 ? 64 : 8));
    if (p.tw) {
        p.ring_off = (int)((p.lds_bytes + 15) / 16 * 16);
        p.lds_bytes = (size_t)p.ring_off + 2048;
    }
    if (p.lds_bytes > kLdsBytes) return plan_fail(err, MI_EUNSUPPORTED, "csr_rank1: n = %d exceeds the state LDS budget", f.n);
    p.grid = run.R; p.block = p.tw ? 128 : 64;
    *out = p;
    return MI_OK;
}

// K2p: two replicas per wavefront -- half the adjacency traffic per update.  Which of its packings the kernel reads:
// trimmed rows and 16-bit neighbour words wherever the model has them, the options allow them and the form is built
inline int plan_k2p(const SlotModelFacts &f, const RunFacts &run, const PlanOptions &o, bool tw, AnnealPlan *out, std::string *err)
{
    AnnealPlan p;
    p.family = PLAN_K2P; p.D = f.D; p.weighted = run.pair_weight_slot >= 0;
    // the ring costs LDS: beyond 64 slots only seven workgroups (14 replicas) fit a CU, and a run that fills the chip
    // (16 replicas per CU) would take two rounds -- such models keep the kernel without a threshold wavefront
    if (tw && ((size_t)f.slots * 256 + 4096) * 8 > kLdsBytes && run.R > 2 * 7 * 256) tw = false;
    const bool trim = o.k2_trim != 2 && f.trim_rw != 0, n16 = o.k2_nbr16 != 2 && f.has_pair16;
    if (p.weighted) {                         // pair-term weights (16 entries per variable)
        if (f.D != 16) return plan_fail(err, MI_EUNSUPPORTED, "csr_rank1 pair kernel: pair-term weights at slot-ELL width %d not built", f.D);
        p.packing = PACK_PAIR; p.adj_bytes = 8448; p.tw = tw;
    } else if (f.D == 16 && tw && trim) {     // rows of at most 15 entries: the trimmed packings (see the kernel)
        p.tw = true; p.trim_rw = f.trim_rw; p.nbr16 = n16;
        p.packing = n16 ? PACK_PAIR16_TRIM : PACK_PAIR_TRIM;
        p.adj_bytes = n16 ? 6144 : (f.trim_rw == 15 ? 7936 : (f.trim_rw == 14 ? 7424 : 6912));
    } else if (n16 && ((f.D == 16 && tw) || f.D == 32)) {   // full rows, 16-bit neighbour words (+ the dword of linear terms)
        p.tw = f.D == 16; p.nbr16 = true; p.packing = PACK_PAIR16;
        p.adj_bytes = f.D == 16 ? 6400 : 12544;
    } else {
        if (f.D != 16 && f.D != 32) return plan_fail(err, MI_EUNSUPPORTED, "csr_rank1 pair kernel: slot-ELL width %d not built", f.D);
        p.tw = tw && f.D == 16; p.packing = PACK_PAIR;
        p.adj_bytes = f.D == 16 ? 8448 : 16640;
    }
    // 4 bytes per variable; tw: the two-deep ring of thresholds behind them (2 x 4 slots x 64 lanes x 8 bytes)
    p.lds_bytes = (size_t)f.slots * 256 + (p.tw ? 4096 : 0);
    if (p.lds_bytes > kLdsBytes) return plan_fail(err, MI_EUNSUPPORTED, "csr_rank1 pair kernel: n = %d exceeds the state LDS budget", f.n);
    p.grid = (run.R + 1) / 2; p.block = p.tw ? 128 : 64;
    *out = p;
    return MI_OK;
}

// K2w: one wavefront per replica sweeps spb = 1 / 2 / 4 slots per step (a model whose every block of 64 spb seats is free of
// internal edges; the pair packing)
inline int plan_k2w(const SlotModelFacts &f, const RunFacts &run, int spb, bool tw, AnnealPlan *out, std::string *err)
{
    AnnealPlan p;
    p.family = PLAN_K2W; p.D = f.D; p.step = spb; p.tw = tw; p.packing = PACK_PAIR; p.weighted = run.pair_weight_slot >= 0;
    const bool d16 = f.D == 16, d32 = f.D == 32;
    if (p.weighted && !(tw && (d16 || d32) && spb == 1))    // pair-term weights: one slot per step beside a threshold wavefront
        return plan_fail(err, MI_EUNSUPPORTED, "csr_rank1 wide kernel: a model with pair-term weights runs one slot per step beside a threshold wavefront");
    const bool built = tw ? ((d16 && (spb == 1 || spb == 2 || spb == 4)) || (d32 && (spb == 1 || spb == 2)))
                          : ((d16 && (spb == 2 || spb == 4)) || (d32 && spb == 2));
    if (!built)
        return plan_fail(err, MI_EUNSUPPORTED, "csr_rank1 wide kernel: width %d / %d slots per step%s not built", f.D, spb, tw ? " with a threshold wavefront" : "");
    p.lds_bytes = (size_t)f.slots * 256 + (tw ? 2048 : 0);    // the cells; tw: + the ring of thresholds
    if (p.lds_bytes > kLdsBytes) return plan_fail(err, MI_EUNSUPPORTED, "csr_rank1 wide kernel: n = %d exceeds the state LDS budget", f.n);
    if (f.slots % spb != 0) return plan_fail(err, MI_EINVAL, "csr_rank1 wide kernel: %d slots are not whole blocks of %d", f.slots, spb);
    p.grid = run.R; p.block = tw ? 128 : 64;
    *out = p;
    return MI_OK;
}

// K2s: a workgroup of nw = 1 / 2 / 4 wavefronts per replica (the pair packing of a model whose every block of 64 nw seats is
// free of internal edges)
inline int plan_k2s(const SlotModelFacts &f, const RunFacts &run, int nw, AnnealPlan *out, std::string *err)
{
    AnnealPlan p;
    p.family = PLAN_K2S; p.D = f.D; p.step = nw; p.packing = PACK_PAIR;
    if (!((f.D == 16 || f.D == 32) && (nw == 1 || nw == 2 || nw == 4)))
        return plan_fail(err, MI_EUNSUPPORTED, "csr_rank1 split kernel: width %d / %d wavefronts not built", f.D, nw);
    p.lds_bytes = (size_t)f.slots * 256 + kCommBytes + (nw > 1 ? kRingBytes : 0);
    if (p.lds_bytes > kLdsBytes) return plan_fail(err, MI_EUNSUPPORTED, "csr_rank1 split kernel: n = %d exceeds the state LDS budget", f.n);
    if (f.slots % nw != 0) return plan_fail(err, MI_EINVAL, "csr_rank1 split kernel: %d slots are not whole blocks of %d", f.slots, nw);
    if (nw > 1 && f.slots % 4 != 0)
        return plan_fail(err, MI_EINVAL, "csr_rank1 split kernel: with %d wavefronts per replica the slots (%d) must come in whole groups of four", nw, f.slots);
    p.grid = run.R; p.block = 64 * nw;
    *out = p;
    return MI_OK;
}

// Which of the kernels of the structured binary model (all run the same chain): an explicit option first; otherwise few
// replicas -> K2s / K2w in its one-wavefront form (random words a few rounds per step, 32-bit state cells: 5 % faster than
// K2 / K2p when every wavefront has a SIMD to itself; its 2 / 4-wavefront forms only on request: measured break-even),
// more replicas than the chip has SIMDs -> two replicas per wavefront, else one
inline int plan_csr_rank1(const SlotModelFacts &f, const RunFacts &run, const PlanOptions &o, AnnealPlan *out, std::string *err)
{
    const int R = run.R;
    const bool pair_ok = f.has_pair_packing, split_ok = f.free_block >= 64 && pair_ok;
    const bool tw = o.k2_tw != 2;                // a threshold wavefront beside the sweeping one (same chain)
    // these kernels keep 4 bytes of LDS per seat: the library's own choice takes them only when the workgroups of
    // the run are resident in ONE round (else K2 with its bit / byte state, 16 replicas per CU at any size)
    const long cus = run.cus > 0 ? run.cus : 256;
    auto one_round = [&](size_t lds_per_wg, long wgs) {
        return lds_per_wg * (size_t)((wgs + cus - 1) / cus) <= kLdsBytes;
    };
    const size_t cells = (size_t)f.slots * 256;
    // K2p: with its threshold wavefront 8 workgroups (16 replicas) fill a CU -- for runs of up to that many; beyond,
    // the kernel without it holds 16 workgroups per CU (6144 replicas: 4.3e11 against two rounds at 3.5e11).  Models
    // of up to 4608 variables keep 8 workgroups' cells per CU at any replica count (several rounds if need be);
    // larger ones take K2p only when one round holds the run.
    const long pair_wgs = ((long)R + 1) / 2;
    const long tw_rounds = (pair_wgs + 8 * cus - 1) / (8 * cus);
    const bool tw_pair = tw && f.D == 16 &&
                         ((pair_wgs <= 8 * cus && one_round(cells + 4096, pair_wgs)) ||            // one round, or
                          (10 * pair_wgs >= 9 * tw_rounds * 8 * cus && (cells + 4096) * 8 <= kLdsBytes));   // nearly full ones
    const bool pair_run = pair_ok && (cells * 8 <= (size_t)150 * 1024 || one_round(cells + (tw_pair ? 4096 : 0), pair_wgs));
    int choice = 0;                              // 0: K2, 1: K2p, 2: K2w / K2s
    // (a model with pair-term weights: the kernels that sweep its weighted slot are K2, K2p and K2w with one slot
    // per step beside a threshold wavefront)
    const bool weighted = run.pair_weight_slot >= 0;
    if (weighted) {
        if (o.k2_pair != 2 && pair_run && f.D == 16 && R > 1024) choice = 1;
        else if (o.k2_split != 2 && tw && o.k2_wide != 2 && split_ok && R <= o.k2_split_max && one_round(cells + 2048, R)) choice = 2;
    } else if (o.k2_split == 1 && split_ok) choice = 2;
    else if (o.k2_pair == 1 && pair_ok) choice = 1;
    else if (o.k2_split != 2 && split_ok && R <= o.k2_split_max && one_round(cells + 2048, R)) choice = 2;
    else if (o.k2_pair != 2 && pair_run && R > 1024) choice = 1;

    if (choice == 2 && weighted)                 // (an edge-free layout in wider blocks is one in 64-seat slots too)
        return plan_k2w(f, run, 1, true, out, err);
    if (choice == 2 && f.free_block > 64 && o.k2_wide != 2 && (f.D == 16 || f.free_block == 128))
        return plan_k2w(f, run, f.free_block / 64, tw, out, err);   // blocks of 128 / 256 edge-free seats, few replicas: ONE wavefront sweeps a block per step
    if (choice == 2 && f.free_block == 64 && o.k2_wide != 2 && tw)
        return plan_k2w(f, run, 1, true, out, err);                 // 64-seat layouts: one slot per step, thresholds from the second wavefront
    if (choice == 2) return plan_k2s(f, run, f.free_block / 64, out, err);
    if (choice == 1)                             // (forced: a threshold wavefront whenever one round of 8 workgroups per CU holds the run)
        return plan_k2p(f, run, o, o.k2_pair == 1 ? (tw && f.D == 16 && pair_wgs <= 8 * cus) : tw_pair, out, err);
    // K2: every wavefront alone on its SIMD (up to 1024 replicas) -> a threshold wavefront beside it
    return plan_k2(f, run, tw && R <= 1024, out, err);
}

// K3f serves every slot-edge-free Potts model of 16 / 32 entries per variable and 2..16 cases (the kernels with the
// minimum-size test are built too); everything else runs on K3
inline int plan_potts(const SlotModelFacts &f, const RunFacts &run, const PlanOptions &o, AnnealPlan *out, std::string *err)
{
    AnnealPlan p;
    p.weighted = run.node_weights;               // node weights (chain 2d)
    if (f.has_fast_packing && o.k3_fast != 2 && (f.D == 16 || f.D == 32) && f.K >= 2 && f.K <= 16) {
        p.family = PLAN_K3F; p.D = f.D; p.packing = PACK_FAST;
        p.KM = f.K <= 8 ? 8 : 16;
        // (up to 1024 replicas every wavefront has a SIMD to itself: a threshold wavefront beside each)
        p.tw = o.k2_tw != 2 && run.R <= 1024;
        p.size_test = run.min_cluster_size > 0;
        if (p.weighted && p.size_test) return plan_fail(err, MI_EUNSUPPORTED, "node weights with min_cluster_size are not supported");
        p.lds_bytes = (size_t)f.slots * 128 + 256 + (p.tw ? 4096 : 0);   // 2 bytes per seat + the cluster sizes (+ the ring)
        if (p.lds_bytes > kLdsBytes) return plan_fail(err, MI_EUNSUPPORTED, "potts fast kernel: n = %d exceeds the label LDS budget", f.n);
        p.grid = run.R; p.block = p.tw ? 128 : 64;
    } else {
        p.family = PLAN_K3; p.D = f.D <= 64 ? f.D : 0;
        if (!ell_width_built(f.D)) return plan_fail(err, MI_EUNSUPPORTED, "slot-ELL width %d not built", f.D);
        const size_t per_wave = (size_t)f.slots * 64 + 256;          // labels + cluster sizes
        p.step = 4;                              // wavefronts (replicas) per workgroup; fewer when their LDS state is large
        while (p.step > 1 && per_wave * p.step > kLdsBytes) --p.step;
        p.lds_bytes = per_wave * p.step;
        if (p.lds_bytes > kLdsBytes)
            return plan_fail(err, MI_EUNSUPPORTED, "model too large for the LDS-resident sparse kernel (%zu B)", p.lds_bytes);
        p.grid = (run.R + p.step - 1) / p.step; p.block = p.step * 64;
    }
    *out = p;
    return MI_OK;
}

inline int plan_anneal(const SlotModelFacts &f, const RunFacts &run, const PlanOptions &o, AnnealPlan *out, std::string *err)
{
    return f.kind == MI_KIND_POTTS_CSR ? plan_potts(f, run, o, out, err) : plan_csr_rank1(f, run, o, out, err);
}

// the name mi_sa_last_kernel_name reports for the kernel of a plan
inline void plan_kernel_name(const AnnealPlan &p, char *buf, size_t len)
{
    const char *tw = p.tw ? ", tw" : "";
    switch (p.family) {
    case PLAN_K2: snprintf(buf, len, "k_anneal_csr_rank1<%d, %d%s>", p.D, p.state_bytes, tw); break;
    case PLAN_K2P:
        if (p.trim_rw) snprintf(buf, len, "k_anneal_csr_rank1_pair<%d, tw> r%d", p.D, p.trim_rw);
        else snprintf(buf, len, "k_anneal_csr_rank1_pair<%d%s>", p.D, tw);
        break;
    case PLAN_K2W: snprintf(buf, len, "k_anneal_csr_rank1_wide<%d, %d%s>", p.D, p.step, tw); break;
    case PLAN_K2S: snprintf(buf, len, "k_anneal_csr_rank1_split<%d, %d>", p.D, p.step); break;
    case PLAN_K3: snprintf(buf, len, "k_anneal_potts<%d%s>", p.D, p.weighted ? ", weighted" : ""); break;
    case PLAN_K3F: snprintf(buf, len, "k_anneal_potts_fast<%d, %d%s%s>", p.D, p.KM, tw, p.weighted ? ", weighted" : ""); break;
    default: snprintf(buf, len, "?"); break;
    }
}

}  // namespace mi_sa_plan
