// mi_sa.hip -- MI355X (gfx950) simulated-annealing engine: kernels + C ABI (include/mi_sa.h).
//
// Chain specification (shared with the CPU oracle by DESIGN.md, not by code):
//   * dense binary model  E(x) = x^T Qs x + offset.  Device matrix Q2 = 2*Qs off-diagonal, 0 on the
//     diagonal; diag = Qs_ii.  Cached local field f_i = diag_i + sum_j Q2_ij x_j.
//   * proposal (variable i, sweep s, global replica g): accepted iff
//         (x_i ? -f_i : f_i)  <  neglog_u(philox(i, s, g, 0)) * T_s ,   T_s = (float)(1/beta_s)
//     variables visited in index order 0..n-1; an accepted flip adds +-Q2 row i to f.
//   * one 64-lane wavefront owns one replica.  Variable i lives on lane (i & 63), slot t = i >> 6;
//     the field of slot t is VGPR f[t] (fully unrolled, NT slots).  Within a slot all 64 lanes test
//     their proposal at once; the LOWEST accepting lane is committed, its Q2 row is streamed
//     (16 B/lane coalesced loads from the slot-permuted matrix) into f, and only lanes above it are
//     re-tested -- exactly the sequential sweep order of the oracle, with rejected proposals free.
//
// Reference call sites served: BQM_clustering.py:57,75,85,245,263,273,386 ; DQM_clustering.py:45.

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/mi_sa.h"

#include "mi_sa_device.h"
#include "mi_sa_pack.h"

namespace mi_sa_impl {

// ------------------------------------------------------------------------------------------------
// error plumbing
// ------------------------------------------------------------------------------------------------
thread_local std::string g_err;

thread_local std::string g_kernel;

void note_kernel(const char *fmt, ...)
{
    char buf[128];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (g_kernel.find(buf) == std::string::npos) g_kernel += (g_kernel.empty() ? "" : " + ") + std::string(buf);
}

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}



// ------------------------------------------------------------------------------------------------
// K5: best-of-replicas: packed (sortable(float E) << 32 | global id) minimum
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sortable_f32(float v)
{
    const uint32_t b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// One workgroup: the replica with the lowest fp64 energy (ties: the lowest index) -- exactly the record a sorted
// SampleSet puts first.  The packed key it writes for the cross-GPU exchange carries float(E): between GPUs the
// comparison has fp32 resolution (1 part in 1.7e7 of |E|), inside one GPU it is exact.
__global__ void __launch_bounds__(1024) k_best(const double *__restrict__ energy, int R,
                                               uint32_t replica_offset,
                                               unsigned long long *__restrict__ out_key)
{
    __shared__ double s_e[16];
    __shared__ int s_i[16];
    double be = INFINITY;
    int bi = 0x7fffffff;
    for (int r = threadIdx.x; r < R; r += blockDim.x) {
        const double e = energy[r];
        if (e < be || (e == be && r < bi)) { be = e; bi = r; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double oe = __shfl_xor(be, off, 64);
        const int oi = __shfl_xor(bi, off, 64);
        if (oe < be || (oe == be && oi < bi)) { be = oe; bi = oi; }
    }
    if ((threadIdx.x & 63) == 0) { s_e[threadIdx.x >> 6] = be; s_i[threadIdx.x >> 6] = bi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
            if (s_e[w] < be || (s_e[w] == be && s_i[w] < bi)) { be = s_e[w]; bi = s_i[w]; }
        if (bi == 0x7fffffff) bi = 0;                       // every energy NaN: report replica 0
        out_key[0] = ((unsigned long long)sortable_f32((float)energy[bi]) << 32) |
                     (unsigned long long)(replica_offset + (uint32_t)bi);
    }
}

// ------------------------------------------------------------------------------------------------
// K6: replica exchange of parallel tempering, on the device
// ------------------------------------------------------------------------------------------------
// R = chains x T replicas, global replica g belongs to chain g / T and holds ladder rung rung[g].  One workgroup per
// chain.  Round `rnd` proposes the disjoint neighbour pairs (k, k+1), k = (rnd & 1), +2, ...: with a, b the replicas
// holding rungs k and k+1,
//     arg = (beta_k - beta_{k+1}) (E_a - E_b)                       (fp64)
//     exchange iff  arg >= 0  or  -arg < neglog_u(word(i = chain T + k, s = rnd, g = 0xffffffff, tag 3))
// -- Metropolis, min(1, e^arg), with the chain's own bit-reproducible logarithm and Philox stream, so every GPU
// (and the oracle, oracle/pt_oracle.py) takes the same decisions from the same energies.  Temperatures move, states
// never do: the kernel swaps the two rung indices and rewrites temps[] of the replicas this GPU owns.
__global__ void __launch_bounds__(256) k_pt_exchange(const double *__restrict__ energy, int *__restrict__ rung,
                                                     const double *__restrict__ betas,
                                                     const float *__restrict__ ladder_temps,
                                                     float *__restrict__ temps_local, int T, int lo, int hi,
                                                     uint32_t rnd, uint32_t seed_lo, uint32_t seed_hi,
                                                     unsigned long long *__restrict__ stats)
{
    extern __shared__ int holder[];                          // holder[k] = replica of this chain on rung k
    const int c = blockIdx.x;
    for (int t = threadIdx.x; t < T; t += blockDim.x) holder[rung[c * T + t]] = c * T + t;
    __syncthreads();
    unsigned int proposed = 0, accepted = 0;
    for (int k = (int)(rnd & 1u) + 2 * (int)threadIdx.x; k + 1 < T; k += 2 * (int)blockDim.x) {
        const int a = holder[k], b = holder[k + 1];
        const double arg = (betas[k] - betas[k + 1]) * (energy[a] - energy[b]);
        ++proposed;
        const bool acc = arg >= 0.0 ||
                         -arg < (double)neglog_u(chain_word_dev((uint32_t)(c * T + k), rnd, 0xffffffffu, 3u, seed_lo, seed_hi));
        if (acc) {
            rung[a] = k + 1;
            rung[b] = k;
            ++accepted;
        }
    }
    __syncthreads();
    for (int t = threadIdx.x; t < T; t += blockDim.x) {
        const int g = c * T + t;
        if (g >= lo && g < hi) temps_local[g - lo] = ladder_temps[rung[g]];
    }
    if (proposed) { atomicAdd(&stats[0], (unsigned long long)proposed); atomicAdd(&stats[1], (unsigned long long)accepted); }
}

}  // namespace mi_sa_impl
using namespace mi_sa_impl;

// ================================================================================================
// host side
// ================================================================================================
// Every d_* member owns its buffer (DevArray, csrc/mi_sa_host.h): deleting the problem frees them.  Members are destroyed
// in reverse order of declaration, so the stream and the two events stand first: buffers go, then events, then the stream.
struct mi_sa_problem {
    int kind = 0, n = 0, K = 0, device = 0, cus = 0;
    double offset = 0.0;
    size_t state_elem = 1;
    ScopedStream stream;
    Events<2> ev;                                // around the kernels of the last anneal
    struct Dense {                               // n <= 4096
        int NT = 0;
        DevArray<float> d_Qp;
        DevArray<float> d_Qm;                    // K1m: plain row-major Q2 + diagonal row (NT <= 44)
        DevArray<float> d_fields;                // cached fields between the launches of a run that is cut (DensePlan::field_floats)
        DevArray<unsigned int> d_ctrl;           // kernel-scheduling words (the scheduled form)
        int resident_waves = 0;                  // co-resident wavefronts of K1 on this device (0: not asked yet)
    } dense;
    struct DenseXl {                             // n > 4096: the model and the state of a run
        int chunks = 0;
        DevArray<float> d_Q2, d_diag;            // K1x: padded rows of 2*Qs, diagonal
        DevArray<uint8_t> d_xg;                  // K1g workspace in bytes (fields of all replicas, state words, signs, thresholds)
        std::thread worker;                      // joined by the next call on this problem (settle)
        int worker_rc = MI_OK;
        std::string worker_err, worker_kernel;
    } xl;
    struct Slot {                                // structured kinds (slot-ELL)
        int slots = 0, D = 0;
        float c_pair = 0.0f;
        DevArray<uint32_t> d_ell_col;
        DevArray<float> d_ell_val, d_lin;
        DevArray<double> d_ell_val64, d_lin64;   // optional fp64 energy model (mi_sa_problem_set_energy_model_f64)
        double c_pair64 = 0.0;
        std::vector<int32_t> h_rowptr;           // the CSR row pointers given at creation
        DevArray<uint2> d_rows;                  // K2: row-major adjacency, in-slot neighbours first
        DevArray<uint32_t> d_meta;               // K2 / K3: in-slot count | degree << 8 | absent << 31
        std::vector<uint32_t> h_meta;            // host copy (mi_sa_problem_set_absent)
        std::vector<uint8_t> h_hole;             // structured binary: positions whose linear term is +inf (mi_sa_problem_set_pair_weights)
        SlotModelFacts facts;                    // what the model is eligible for (csrc/mi_sa_plan.h): which of the packings below exist
        DevArray<uint32_t> d_adj4;               // K2: packed slot adjacency (see EllArgs::adj4)
        DevArray<uint32_t> d_adj4p;              // facts.has_pair_packing: the same with neighbour word = 4 * index (K2p, K2w, K2s); facts.has_fast_packing: 2 * index (K3f)
        DevArray<uint32_t> d_adj4r;              // facts.trim_rw: K2p's trimmed packing (pack_pair_adjacency)
        std::vector<uint32_t> h_adj4r;           // ... its host image until the linear terms are in it (RW = 15; mi_sa_problem_create_csr_rank1)
        DevArray<uint32_t> d_adj16;              // K2p: the packing with 16-bit neighbour words (pack_pair_adjacency16); null = not built
        DevArray<uint32_t> d_adj16r;             // ... the same with the linear term in the sixteenth value (rows of 13..15 entries at D = 16)
        std::vector<uint32_t> h_adj16;           // ... its host image until the linear terms are known (mi_sa_problem_create_csr_rank1)
        DevArray<uint32_t> d_slot_flags;         // K2: slots with internal edges
        DevArray<int32_t> d_wgt;                 // K2 family: the 64 pair-term weights of the weighted slot (mi_sa_problem_set_pair_weights)
        int wslot = -1;                          // ... its index; -1: every weight is 1
        const uint4 *packing(int which) const    // the packed adjacency a plan binds to EllArgs::adj4 (PlanPacking)
        {
            const DevArray<uint32_t> *a = &d_adj4;
            switch (which) {
            case PACK_PAIR: case PACK_FAST: a = &d_adj4p; break;
            case PACK_PAIR_TRIM: a = &d_adj4r; break;
            case PACK_PAIR16: a = &d_adj16; break;
            case PACK_PAIR16_TRIM: a = &d_adj16r; break;
            }
            return reinterpret_cast<const uint4 *>(a->p);
        }
    } slot;
    struct NodeWeights {                         // Potts (mi_sa_problem_set_node_weights)
        DevArray<int32_t> d_nwq;                 // node weights of the pair term per position
        DevArray<float> d_ncw;                   // ... their fp32 coefficients
        DevArray<double> d_nw64;                 // ... their fp64 weights (reported energies)
        int ngroups = 1;                         // ... resolution groups (mi_sa_problem_set_node_weight_groups): d_ncw holds ngroups x seats
        DevArray<double> d_gconst;               // ... per group: fp64 pair coefficient, then energy offset [2 x ngroups] (null: c_pair64, offset)
    } nw;
    struct Merge {                               // Potts: the merge phase of chain 2e (mi_sa_problem_set_merge_moves); interval 0 = off
        int interval = 0, proposals = 0;
        std::vector<double> cq;                  // coefficient of W_a W_b per resolution group (empty: c_pair, unweighted)
        DevArray<double> d_cq;                   // ... its device copy (256 slots)
        double sumabs = 0.0;                     // sum of |S_uv| over the stored couplings, in stored order (fixed-point exponent)
    } merge;
    struct Run {                                 // run buffers; d_states, d_energy and d_init hold the same number of replicas (ensure_run_buffers)
        DevArray<float> d_temps;
        DevArray<uint8_t> d_init, d_states;      // in bytes: R x n x state_elem
        DevArray<double> d_energy;
        DevArray<unsigned long long> d_stats;    // 4 words: proposals, accepted, bytes, best-key
        DevArray<unsigned int> d_pace;           // kPaceWords per launch chunk
    } run;
    struct Options {                             // mi_sa_set_option
        int debug = 0;                           // DenseArgs::debug (diagnostic timing only; results are wrong)
        int xl_batched = 0;                      // n > 4096: 0 auto (K1g for >= 256 replicas or n >= 16384), 1 always K1g, 2 always K1x
        int xl_chain = 0;                        // K1g, chain of a group of blocks: 0 auto (fused up to 512 replicas), 1 a DIAG and a small pass per block, 2 fused
        int xl_chunk = 8;                        // K1g: sweeps per chunk of a cooling run (the hand-over to K1x is decided per chunk)
        int xl_cold_permille = 20;               // hand the rest of the run to K1x when a chunk accepted less than this share (0 = never)
        int xl_async = 1;                        // that cooling run is driven by a worker thread: mi_sa_anneal returns at once (0 = in the caller)
        int min_cluster_size = 0;                // K3: hard lower bound on every cluster's size (CQM_clustering.py:46-48)
        PlanOptions plan;                        // the k2_* / k3_* options: what the planner reads (csrc/mi_sa_plan.h)
        DensePlanOptions dense;                  // pace, variant, unit_rows, *_permille, chunk_sweeps: what the dense planner reads (csrc/mi_dense_plan.h)
    } opt;
    struct Tempering {                           // mi_sa_tempering_*: ladder, rung of every replica of the run, exchange statistics
        int T = 0, chains = 0, lo = 0, R_local = 0;
        DevArray<int> d_rung;
        DevArray<double> d_betas, d_energy;
        DevArray<float> d_ladder;
        DevArray<float> d_temps;                 // per-replica temperatures of the next tempering round (its own buffer: an ordinary anneal on the same handle rewrites run.d_temps)
        DevArray<unsigned long long> d_stats;
        void clear()                             // no tempering set up
        {
            T = 0;
            d_rung.reset(); d_betas.reset(); d_energy.reset(); d_ladder.reset(); d_temps.reset(); d_stats.reset();
        }
    } pt;
    struct Last {                                // what the last anneal was
        int R = 0;
        uint32_t offset = 0;
        bool has_run = false;
        int adj_bytes = 0;                       // packed adjacency bytes a wavefront fetched per slot (0: a kernel without such a packing)
        int launches = 1;                        // kernel launches that served it
        std::string kernel;                      // ... and the kernel(s) they ran
    } last;
};

namespace {

constexpr int kMaxDenseXlN = 16 * 4096;    // workgroup-per-replica kernel (K1x)

// d_states, d_energy and d_init (where it exists) always hold the same number of replicas, d_energy.count: growing resets
// all three before it allocates any, so after a failure each is empty or of the new size, and the next call (which sees
// d_energy empty) starts over.
int ensure_run_buffers(mi_sa_problem *p, int R, int num_sweeps, bool need_init)
{
    mi_sa_problem::Run &b = p->run;
    const size_t replica_bytes = (size_t)p->n * p->state_elem;
    if ((size_t)R > b.d_energy.count) {
        b.d_states.reset(); b.d_init.reset(); b.d_energy.reset();
        HIP_TRY(b.d_states.resize((size_t)R * replica_bytes));
        HIP_TRY(b.d_energy.resize((size_t)R));
    }
    if (need_init) HIP_TRY(b.d_init.reserve(b.d_energy.count * replica_bytes));
    HIP_TRY(b.d_temps.reserve((size_t)(num_sweeps > 0 ? num_sweeps : 0)));
    return MI_OK;
}

// what the translation unit of a register width exports (csrc/dense_kernels.hip)
DenseWidth dense_width_unit(int NT)
{
    switch (NT) {
#define MI_CASE(N) case N: return mi_dense_nt##N();
        MI_CASE(4) MI_CASE(8) MI_CASE(12) MI_CASE(16) MI_CASE(20) MI_CASE(24) MI_CASE(28)
        MI_CASE(32) MI_CASE(36) MI_CASE(40) MI_CASE(44) MI_CASE(48) MI_CASE(52) MI_CASE(56)
        MI_CASE(60) MI_CASE(64)
#undef MI_CASE
    }
    return DenseWidth{nullptr, nullptr, nullptr};
}

// A cooling run on the batched large-model kernels decides its hand-over per chunk on the host (anneal_dense_xl), in a
// worker thread of the problem.  Every entry point that takes the problem joins that thread first; its error becomes the
// error of the joining call, and the run that failed counts as not run.
int settle(mi_sa_problem *p)
{
    if (!p->xl.worker.joinable()) return MI_OK;
    p->xl.worker.join();
    p->last.kernel = p->xl.worker_kernel;
    if (p->xl.worker_rc) {
        const int rc = p->xl.worker_rc;
        p->xl.worker_rc = MI_OK;
        p->last.has_run = false;
        return fail(rc, "%s", p->xl.worker_err.c_str());
    }
    return MI_OK;
}

// The one way into an entry point on a problem, always in this order: no exception leaves it; the problem (and, where
// the entry has other pointer arguments, args_ok) is not null; the worker is joined; then what `need` asks for: a
// finished run, the problem's device current, its stream idle.
enum : unsigned { NEED_RUN = 1, ON_DEVICE = 2, STREAM_IDLE = 4 | ON_DEVICE };
constexpr int NO_ARGS = -1;                // args_ok of an entry whose only pointer argument is the problem

template <typename F>
int on_problem(mi_sa_problem *p, int args_ok, unsigned need, F &&body)
{
    return guarded([&]() -> int {
        if (!p || !args_ok) return fail(MI_EINVAL, args_ok == NO_ARGS ? "NULL problem" : "NULL argument");
        MI_TRY(settle(p));
        if ((need & NEED_RUN) && !p->last.has_run) return fail(MI_ESTATE, "no anneal has been run on this problem");
        if (need & ON_DEVICE) HIP_TRY(hipSetDevice(p->device));
        if ((need & STREAM_IDLE) == STREAM_IDLE) HIP_TRY(hipStreamSynchronize(p->stream));
        return body();
    });
}

// What every create shares: the device check, the handle with its stream, events and fixed buffers, then the kind's own
// `fill`.  A failure anywhere releases through mi_sa_problem_destroy.
template <typename F>
int new_problem(int kind, int n, int K, double offset, size_t state_elem, int device, mi_sa_problem **out, F &&fill)
{
    MI_TRY(pick_device(device));
    mi_sa_problem *p = new (std::nothrow) mi_sa_problem();
    if (!p) return fail(MI_ENOMEM, "out of host memory");
    p->kind = kind; p->n = n; p->K = K; p->offset = offset; p->state_elem = state_elem; p->device = device;
    const int rc = guarded([&]() -> int {
        HIP_TRY(hipStreamCreateWithFlags(&p->stream.st, hipStreamNonBlocking));
        for (hipEvent_t &e : p->ev.e) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(p->run.d_stats.resize(16));
        HIP_TRY(hipMemset(p->run.d_stats, 0, 16 * sizeof(unsigned long long)));
        HIP_TRY(p->run.d_pace.resize(kMaxChunks * kPaceWords));
        HIP_TRY(hipDeviceGetAttribute(&p->cus, hipDeviceAttributeMultiprocessorCount, device));
        return fill(p);
    });
    if (rc) { mi_sa_problem_destroy(p); return rc; }
    *out = p;
    return MI_OK;
}

// K1x: Q stays in HBM as n padded rows of 2*Qs (zero diagonal), uploaded in blocks of rows
int upload_dense_xl(mi_sa_problem *p, const float *Qs)
{
    const int n = p->n;
    p->xl.chunks = (n + 4095) / 4096;
    const size_t xstride = (size_t)p->xl.chunks * 4096;
    HIP_TRY(p->xl.d_Q2.resize((size_t)n * xstride));
    const int rows_per_block = 256;
    std::vector<float> blk((size_t)rows_per_block * xstride), hd(xstride, 0.0f);
    for (int r0 = 0; r0 < n; r0 += rows_per_block) {
        const int nr = n - r0 < rows_per_block ? n - r0 : rows_per_block;
        std::fill(blk.begin(), blk.begin() + (size_t)nr * xstride, 0.0f);
        for (int i = 0; i < nr; ++i) {
            const float *row = Qs + (size_t)(r0 + i) * n;
            float *dst = blk.data() + (size_t)i * xstride;
            for (int j = 0; j < n; ++j) dst[j] = row[j] + row[j];
            dst[r0 + i] = 0.0f;
            hd[r0 + i] = row[r0 + i];
        }
        HIP_TRY(hipMemcpy(p->xl.d_Q2 + (size_t)r0 * xstride, blk.data(), (size_t)nr * xstride * sizeof(float), hipMemcpyHostToDevice));
    }
    HIP_TRY(p->xl.d_diag.upload(hd));
    return MI_OK;
}

int upload_dense(mi_sa_problem *p, const float *Qs)
{
    const int n = p->n, slots = (n + 63) / 64;
    const int NT = p->dense.NT = ((slots + 3) / 4) * 4;
    const size_t stride = (size_t)NT * 64;
    // host-side permute: Qp[i][(g*64+lane)*4+c] = 2*Qs[i][64*(4g+c)+lane] (0 on diagonal / padding)
    const int diag_row = slots * 64;
    std::vector<float> hp((size_t)(diag_row + 1) * stride, 0.0f);
    for (int i = 0; i < n; ++i) {
        const float *row = Qs + (size_t)i * n;
        float *dst = hp.data() + (size_t)i * stride;
        for (int j = 0; j < n; ++j) {
            if (j == i) continue;
            const int t = j >> 6, lane = j & 63;
            dst[((size_t)(t >> 2) * 64 + lane) * 4 + (t & 3)] = row[j] + row[j];
        }
        hp[(size_t)diag_row * stride + ((size_t)((i >> 6) >> 2) * 64 + (i & 63)) * 4 + ((i >> 6) & 3)] = row[i];
    }
    HIP_TRY(p->dense.d_Qp.upload(hp));
    if (NT <= kMaxMfmaNT) {
        // K1m layout: plain row-major Q2 (zero diagonal), NPAD = 64*NT columns, NPAD rows + the diagonal row
        const size_t npad = (size_t)NT * 64;
        std::vector<float> hm((npad + 1) * npad, 0.0f);
        for (int i = 0; i < n; ++i) {
            const float *row = Qs + (size_t)i * n;
            float *dst = hm.data() + (size_t)i * npad;
            for (int j = 0; j < n; ++j) dst[j] = (j == i) ? 0.0f : row[j] + row[j];
            hm[npad * npad + i] = row[i];
        }
        HIP_TRY(p->dense.d_Qm.upload(hm));
    }
    return MI_OK;
}

// CSR (both directions stored) -> slot-ELL device arrays (D = 16 / 32 / 64)
int upload_slot_ell(mi_sa_problem *p, const int32_t *rowptr, const int32_t *col, const float *val, int n)
{
    mi_sa_problem::Slot &m = p->slot;
    // what the model is eligible for decides which packings are built (MI_K2_STATE = bit | byte | half narrows K2's state)
    std::string err;
    if (const int rc = slot_model_facts(p->kind, rowptr, col, n, p->K, getenv("MI_K2_STATE"), &m.facts, &err)) return fail(rc, "%s", err.c_str());
    const SlotModelFacts &f = m.facts;
    const int D = f.D, slots = f.slots;
    std::vector<uint32_t> hc;
    std::vector<float> hv;
    build_slot_ell(rowptr, col, val, n, slots, D, hc, hv);
    HIP_TRY(m.d_ell_col.upload(hc));
    HIP_TRY(m.d_ell_val.upload(hv));
    m.slots = slots;
    m.D = D;
    m.h_rowptr.assign(rowptr, rowptr + n + 1);
    // row-major copy (K2, K3): neighbours in the variable's own 64-slot first
    std::vector<uint2> hr((size_t)slots * 64 * D);
    std::vector<uint32_t> hm((size_t)slots * 64, 0u);
    for (int i = 0; i < slots * 64; ++i) {
        uint2 *row = hr.data() + (size_t)i * D;
        for (int k = 0; k < D; ++k) row[k] = make_uint2((uint32_t)(i < n ? i : 0), 0u);   // (self, +0.0f)
        if (i >= n) { hm[i] = 0x80000000u; continue; }    // bit 31: no variable at this position (K3 reads it)
        int k = 0, nin = 0;
        for (int pass = 0; pass < 2; ++pass)
            for (int e = rowptr[i]; e < rowptr[i + 1]; ++e) {
                const bool in_slot = (col[e] >> 6) == (i >> 6);
                if (in_slot != (pass == 0)) continue;
                uint32_t bits;
                memcpy(&bits, &val[e], 4);
                row[k++] = make_uint2((uint32_t)col[e], bits);
                nin += in_slot ? 1 : 0;
            }
        hm[i] = (uint32_t)nin | ((uint32_t)k << 8);
    }
    HIP_TRY(m.d_rows.upload(hr));
    HIP_TRY(m.d_meta.upload(hm));
    m.h_meta = hm;
    // the packings the facts name (csrc/mi_sa_pack.h): a slot's register image, groups of four (neighbour word, value)
    // per lane
    if (f.has_fast_packing)          // K3f: the neighbour as the LDS byte address of its 16-bit label cell
        HIP_TRY(m.d_adj4p.upload(pack_groups_of_four(hc, hv, slots, D, [](uint32_t c, int, int) { return 2u * c; })));
    if (p->kind != MI_KIND_CSR_RANK1) return MI_OK;
#ifdef MI_K2_DEBUG_BUILD                  /* timing-only builds, never in the shipped library: conflict-free gathers (wrong chain) */
    const bool debug_linear = getenv("MI_K2_DEBUG_LINEAR") != nullptr;
#else
    constexpr bool debug_linear = false;
#endif
    // K2: the neighbour already translated into where its state lives in LDS
    HIP_TRY(m.d_adj4.upload(pack_groups_of_four(hc, hv, slots, D, [&](uint32_t c, int lane, int k) {
        return debug_linear ? (uint32_t)(lane * 2 + (k * 128) % (slots * 128)) : k2_state_word(c, f.state_bytes); })));
    std::vector<uint32_t> hf((size_t)slots, 0u);              // slots with internal edges
    for (size_t i = 0; i < hm.size(); ++i)
        if (hm[i] & 0xffu) hf[i / 64] = 1u;
    HIP_TRY(m.d_slot_flags.upload(hf));
    if (f.has_pair_packing) {    // K2p, K2w, K2s: the neighbour as the LDS byte address of its 32-bit cell
        HIP_TRY(m.d_adj4p.upload(pack_groups_of_four(hc, hv, slots, D, [&](uint32_t c, int lane, int k) {
            return debug_linear ? (uint32_t)(lane * 4 + (k * 256) % (slots * 256)) : 4u * c; })));
        if (f.has_pair16) m.h_adj16 = pack_pair_adjacency16(hc, hv, slots, D);
        if (f.trim_rw) m.h_adj4r = pack_pair_adjacency(hc, hv, slots, D, f.trim_rw);
        if (f.trim_rw && f.trim_rw != 15) {      // (at 15 it waits for the linear terms: upload_linear_terms)
            HIP_TRY(m.d_adj4r.upload(m.h_adj4r));
            std::vector<uint32_t>().swap(m.h_adj4r);
        }
    }
    return MI_OK;
}

// structured binary: the linear terms, and the packings that carry them
int upload_linear_terms(mi_sa_problem *p, const float *lin)
{
    mi_sa_problem::Slot &m = p->slot;
    const int n = p->n;
    // the lanes past n carry lin = +inf: their dE is +inf, never accepted (K2 has no per-lane bound check)
    std::vector<float> hl((size_t)m.slots * 64, INFINITY);
    for (int i = 0; i < n; ++i) hl[i] = lin[i];
    m.h_hole.assign((size_t)n, 0);
    for (int i = 0; i < n; ++i) m.h_hole[(size_t)i] = std::isinf(lin[i]) ? 1 : 0;
    HIP_TRY(m.d_lin.upload(hl));
    if (!m.h_adj4r.empty()) {
        // K2p's trimmed packing at RW = 15 carries the linear term beside the last three neighbour words (pack_pair_adjacency)
        const size_t slot_words = m.h_adj4r.size() / (size_t)m.slots;
        for (int t = 0; t < m.slots; ++t)
            for (int lane = 0; lane < 64; ++lane)
                memcpy(&m.h_adj4r[(size_t)t * slot_words + 3 * 512 + (size_t)lane * 4 + 3], &hl[(size_t)t * 64 + lane], 4);
        HIP_TRY(m.d_adj4r.upload(m.h_adj4r));
        std::vector<uint32_t>().swap(m.h_adj4r);
    }
    if (!m.h_adj16.empty()) {
        HIP_TRY(m.d_adj16.upload(m.h_adj16));
        if (m.facts.trim_rw) {
            // trimmed rows: the sixteenth value is padding in every row and carries the lane's linear term instead
            for (int t = 0; t < m.slots; ++t)
                for (int lane = 0; lane < 64; ++lane)
                    memcpy(&m.h_adj16[(size_t)t * 1536 + 5 * 256 + (size_t)lane * 4 + 3], &hl[(size_t)t * 64 + lane], 4);
            HIP_TRY(m.d_adj16r.upload(m.h_adj16));
        }
        std::vector<uint32_t>().swap(m.h_adj16);
    }
    return MI_OK;
}

// "key=value,..." with the keys of mi_sa_set_option that `set` takes (the host-only planning entries)
template <typename F>
int parse_option_string(const char *options, F &&set)
{
    for (const char *s = options ? options : ""; *s;) {
        const char *end = strchr(s, ','), *eq = strchr(s, '=');
        if (!end) end = s + strlen(s);
        const std::string key(s, eq && eq < end ? eq : end);
        char *stop = nullptr;
        const long value = eq && eq < end ? strtol(eq + 1, &stop, 10) : 0;
        if (stop != end || stop == eq + 1 || !set(key.c_str(), value)) return fail(MI_EINVAL, "unknown option '%s'", key.c_str());
        s = *end ? end + 1 : end;
    }
    return MI_OK;
}

}  // namespace

extern "C" {

const char *mi_last_error(void) { return g_err.c_str(); }

int mi_abi_version(void) { return 1; }

int mi_device_count(int *out_count)
{
    if (!out_count) return fail(MI_EINVAL, "out_count is NULL");
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess) { *out_count = 0; return fail(MI_ENODEV, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *out_count = cnt;
    return MI_OK;
}

int mi_device_info(int device, char *name, int len, int *out_cus, uint64_t *out_hbm_bytes)
{
    MI_TRY(pick_device(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (name && len > 0) snprintf(name, (size_t)len, "%s (%s)", prop.name, prop.gcnArchName);
    if (out_cus) *out_cus = prop.multiProcessorCount;
    if (out_hbm_bytes) *out_hbm_bytes = (uint64_t)prop.totalGlobalMem;
    return MI_OK;
}

int mi_sa_problem_create_dense_f32(const float *Qs, int n, double offset, int device,
                                   mi_sa_problem **out)
{
    return guarded([&]() -> int {
        if (!Qs || !out) return fail(MI_EINVAL, "NULL argument");
        if (n < 1) return fail(MI_EINVAL, "n must be >= 1 (got %d)", n);
        if (n > kMaxDenseXlN)
            return fail(MI_EUNSUPPORTED, "dense kernels support n <= %d (got %d)", kMaxDenseXlN, n);
        return new_problem(MI_KIND_DENSE, n, 0, offset, 1, device, out,
                           [&](mi_sa_problem *p) -> int { return n > kMaxDenseN ? upload_dense_xl(p, Qs) : upload_dense(p, Qs); });
    });
}

// Host-only planning step (no device is touched): the slot-independent sweep order of the structured kernels.
static int plan_slot_order_impl(const int32_t *rowptr, const int32_t *col, int n, int slot, int64_t *perm)
{
    const int nslots = (n + slot - 1) / slot;
    if (nslots <= 1 || n > (1 << 18)) {                      // the greedy pass is O(n * slots): identity beyond 262144
        for (int i = 0; i < n; ++i) perm[i] = i;
        return MI_OK;
    }
    for (int i = 0; i < n; ++i)
        if (rowptr[i + 1] < rowptr[i]) return fail(MI_EINVAL, "rowptr is not monotone at %d", i);
    // variables by descending degree, ties by index (stable counting sort)
    int maxdeg = 0;
    for (int i = 0; i < n; ++i) maxdeg = std::max(maxdeg, rowptr[i + 1] - rowptr[i]);
    std::vector<int> start((size_t)maxdeg + 2, 0), order((size_t)n);
    for (int i = 0; i < n; ++i) start[(size_t)(maxdeg - (rowptr[i + 1] - rowptr[i])) + 1]++;
    for (int d = 0; d <= maxdeg; ++d) start[(size_t)d + 1] += start[(size_t)d];
    for (int i = 0; i < n; ++i) order[(size_t)start[(size_t)(maxdeg - (rowptr[i + 1] - rowptr[i]))]++] = i;
    std::vector<int> fill((size_t)nslots, 0), cap((size_t)nslots, slot), where((size_t)n, -1), stamp((size_t)nslots, -1);
    cap[(size_t)nslots - 1] = n - slot * (nslots - 1);
    for (int v : order) {
        for (int e = rowptr[v]; e < rowptr[v + 1]; ++e) {
            if (col[e] < 0 || col[e] >= n) return fail(MI_EINVAL, "bad column %d in row %d", col[e], v);
            const int w = where[(size_t)col[e]];
            if (w >= 0) stamp[(size_t)w] = v;                // slot w holds a neighbour of v
        }
        // least filled slot that holds no neighbour (ties: lowest index); one that does only as a last resort
        int best = -1, best_nb = -1;
        for (int s = 0; s < nslots; ++s) {
            if (fill[(size_t)s] >= cap[(size_t)s]) continue;
            if (stamp[(size_t)s] == v) { if (best_nb < 0 || fill[(size_t)s] < fill[(size_t)best_nb]) best_nb = s; }
            else if (best < 0 || fill[(size_t)s] < fill[(size_t)best]) best = s;
        }
        const int s = best >= 0 ? best : best_nb;
        where[(size_t)v] = s;
        fill[(size_t)s]++;
    }
    // by slot, then by original index
    std::vector<int> pos((size_t)nslots + 1, 0);
    for (int i = 0; i < n; ++i) pos[(size_t)where[(size_t)i] + 1]++;
    for (int s = 0; s < nslots; ++s) pos[(size_t)s + 1] += pos[(size_t)s];
    for (int i = 0; i < n; ++i) perm[pos[(size_t)where[(size_t)i]]++] = i;
    return MI_OK;
}

// One greedy pass with `nslots` slots of `slot` seats each (no short last slot: holes may sit anywhere).  Returns the
// number of variables that had to share a slot with a neighbour; where[i] = slot of variable i.
static int greedy_slots(const int32_t *rowptr, const int32_t *col, int n, int slot, int nslots,
                        const std::vector<int> &order, std::vector<int> &where)
{
    std::vector<int> fill((size_t)nslots, 0), stamp((size_t)nslots, -1);
    where.assign((size_t)n, -1);
    int clashes = 0;
    for (int v : order) {
        for (int e = rowptr[v]; e < rowptr[v + 1]; ++e) {
            const int w = where[(size_t)col[e]];
            if (w >= 0) stamp[(size_t)w] = v;                // slot w holds a neighbour of v
        }
        int best = -1, best_nb = -1;
        for (int s = 0; s < nslots; ++s) {
            if (fill[(size_t)s] >= slot) continue;
            if (stamp[(size_t)s] == v) { if (best_nb < 0 || fill[(size_t)s] < fill[(size_t)best_nb]) best_nb = s; }
            else if (best < 0 || fill[(size_t)s] < fill[(size_t)best]) best = s;
        }
        const int s = best >= 0 ? best : best_nb;
        if (best < 0) ++clashes;
        where[(size_t)v] = s;
        fill[(size_t)s]++;
    }
    return clashes;
}

static int plan_slot_layout_impl(const int32_t *rowptr, const int32_t *col, int n, int slot, int max_slots,
                                 int64_t *pos, int *out_slots, int *out_clashes)
{
    const int s0 = (n + slot - 1) / slot;
    if (max_slots < s0) max_slots = s0;
    for (int i = 0; i < n; ++i) {
        if (rowptr[i + 1] < rowptr[i]) return fail(MI_EINVAL, "rowptr is not monotone at %d", i);
        for (int e = rowptr[i]; e < rowptr[i + 1]; ++e)
            if (col[e] < 0 || col[e] >= n) return fail(MI_EINVAL, "bad column %d in row %d", col[e], i);
    }
    if (n > (1 << 18)) {
        // a greedy pass is O(n * slots) and repeats while the layout grows: beyond 262144 variables the packed identity
        // layout is returned (as mi_sa_plan_slot_order does); clashes = variables with a neighbour in their own slot
        int clashes = 0;
        for (int i = 0; i < n; ++i) {
            pos[i] = i;
            for (int e = rowptr[i]; e < rowptr[i + 1]; ++e)
                if (col[e] / slot == i / slot) { ++clashes; break; }
        }
        *out_slots = s0;
        if (out_clashes) *out_clashes = clashes;
        return MI_OK;
    }
    // variables by descending degree, ties by index (stable counting sort) -- as mi_sa_plan_slot_order
    int maxdeg = 0;
    for (int i = 0; i < n; ++i) maxdeg = std::max(maxdeg, rowptr[i + 1] - rowptr[i]);
    std::vector<int> start((size_t)maxdeg + 2, 0), order((size_t)n);
    for (int i = 0; i < n; ++i) start[(size_t)(maxdeg - (rowptr[i + 1] - rowptr[i])) + 1]++;
    for (int d = 0; d <= maxdeg; ++d) start[(size_t)d + 1] += start[(size_t)d];
    for (int i = 0; i < n; ++i) order[(size_t)start[(size_t)(maxdeg - (rowptr[i + 1] - rowptr[i]))]++] = i;
    // fewest slots (from the fully packed count up, +1/8 per try) that leave no edge inside a slot; the packed
    // layout's clashes stay if max_slots does not suffice
    std::vector<int> where, first_where;
    int nslots = s0, clashes = 0, first_clashes = 0;
    for (;;) {
        clashes = greedy_slots(rowptr, col, n, slot, nslots, order, where);
        if (nslots == s0) { first_where = where; first_clashes = clashes; }
        if (clashes == 0) break;
        const int next = nslots + std::max(1, nslots / 8);
        if (next > max_slots) { where = first_where; clashes = first_clashes; nslots = s0; break; }
        nslots = next;
    }
    // Small graphs: when holes were needed, the block count is set by how many COLOURS the graph needs, not by n / slot,
    // and the balanced greedy pass wastes some (10 blocks for a 342-cell cluster that 8 colour).  A saturation-degree
    // colouring (DSATUR: always the uncoloured variable that sees the most colours, ties by degree, then index; lowest
    // colour with a free seat) is tried as well, and kept when it needs fewer blocks -- every block is a dependent step
    // of a sweep, so 8 instead of 10 is 20 % of a small model's kernel time.  O(n^2): graphs up to 2048 variables.
    if (clashes == 0 && nslots > s0 && n <= 2048) {
        const int C = nslots;                                        // only fewer colours than the greedy result are of interest
        std::vector<unsigned char> seen((size_t)n * C, 0);
        std::vector<int> sat((size_t)n, 0), colour((size_t)n, -1), fill2((size_t)C, 0);
        int used = 0;
        bool ok = true;
        for (int step = 0; step < n && ok; ++step) {
            int v = -1;
            for (int u = 0; u < n; ++u) {
                if (colour[(size_t)u] >= 0) continue;
                if (v < 0) { v = u; continue; }
                const int du = rowptr[u + 1] - rowptr[u], dv = rowptr[v + 1] - rowptr[v];
                if (sat[(size_t)u] > sat[(size_t)v] || (sat[(size_t)u] == sat[(size_t)v] && du > dv)) v = u;
            }
            int c = 0;
            while (c < C && (seen[(size_t)v * C + c] || fill2[(size_t)c] >= slot)) ++c;
            if (c >= C) { ok = false; break; }
            colour[(size_t)v] = c;
            fill2[(size_t)c]++;
            used = std::max(used, c + 1);
            if (used >= C) { ok = false; break; }                    // no better than the greedy layout
            for (int e = rowptr[v]; e < rowptr[v + 1]; ++e) {
                const int u = col[e];
                if (!seen[(size_t)u * C + c]) { seen[(size_t)u * C + c] = 1; sat[(size_t)u]++; }
            }
        }
        if (ok && used < nslots && used >= s0) {
            where = colour;
            nslots = used;
        }
    }
    std::vector<int> seat((size_t)nslots, 0);
    for (int i = 0; i < n; ++i) pos[i] = (int64_t)where[(size_t)i] * slot + seat[(size_t)where[(size_t)i]]++;   // by index inside a slot
    *out_slots = nslots;
    if (out_clashes) *out_clashes = clashes;
    return MI_OK;
}

int mi_sa_plan_slot_layout(const int32_t *rowptr, const int32_t *col, int n, int slot, int max_slots,
                           int64_t *out_pos, int *out_slots, int *out_clashes)
{
    if (!rowptr || !out_pos || !out_slots || (n > 0 && rowptr[n] > 0 && !col)) return fail(MI_EINVAL, "NULL argument");
    if (n < 1 || slot < 1) return fail(MI_EINVAL, "n and slot must be >= 1");
    return guarded([&]() -> int { return plan_slot_layout_impl(rowptr, col, n, slot, max_slots, out_pos, out_slots, out_clashes); });
}

int mi_sa_plan_slot_order(const int32_t *rowptr, const int32_t *col, int n, int slot, int64_t *out_perm)
{
    if (!rowptr || !out_perm || (n > 0 && rowptr[n] > 0 && !col)) return fail(MI_EINVAL, "NULL argument");
    if (n < 0 || slot < 1) return fail(MI_EINVAL, "n must be >= 0 and slot >= 1");
    return guarded([&]() -> int { return plan_slot_order_impl(rowptr, col, n, slot, out_perm); });
}

int mi_sa_plan_dense(int n, int R, int num_sweeps, int resync_interval, uint32_t flags, int cus, int resident_waves,
                     const char *options, char *out_kernel, int len, int *out_launches, uint64_t *out_field_bytes)
{
    if (!out_kernel || len < 1) return fail(MI_EINVAL, "NULL argument");
    if (flags & ~(uint32_t)(MI_F_CONTINUE | MI_F_BETA_PER_REPLICA | MI_F_TEMPS_RESIDENT | MI_F_BETA_PER_GROUP))
        return fail(MI_EINVAL, "unknown flags 0x%x", flags);
    if (n < 1) return fail(MI_EINVAL, "n must be >= 1 (got %d)", n);
    if (R < 1) return fail(MI_EINVAL, "R must be >= 1 (got %d)", R);
    if (num_sweeps < 0) return fail(MI_EINVAL, "num_sweeps must be >= 0");
    if (resync_interval < 0) return fail(MI_EINVAL, "resync_interval must be >= 0");
    return guarded([&]() -> int {
        DensePlanOptions opts;
        MI_TRY(parse_option_string(options, [&](const char *key, long value) { return dense_plan_option_set(opts, key, value); }));
        DenseRun run;
        run.n = n; run.R = R; run.num_sweeps = num_sweeps; run.resync = resync_interval;
        run.temps_per_replica = (flags & (MI_F_BETA_PER_REPLICA | MI_F_TEMPS_RESIDENT)) != 0;
        run.cus = cus; run.resident_waves = resident_waves;
        std::string err;
        int launches = 1;
        uint64_t field_bytes = 0;
        DensePlan plan;
        if (const int rc = plan_dense(run, opts, &plan, &err)) return fail(rc, "%s", err.c_str());
        dense_plan_kernel_name(plan, out_kernel, (size_t)len);
        launches = plan.launches;
        field_bytes = (uint64_t)plan.field_floats * sizeof(float);
        if (out_launches) *out_launches = launches;
        if (out_field_bytes) *out_field_bytes = field_bytes;
        return MI_OK;
    });
}

int mi_sa_plan_anneal(int kind, const int32_t *rowptr, const int32_t *col, int n, int K, int R, int cus, const char *options,
                      int pair_weight_slot, int node_weights, int min_cluster_size, char *out_kernel, int len,
                      int *out_adjacency_bytes)
{
    if (!rowptr || !out_kernel || len < 1 || (n > 0 && rowptr[n] > 0 && !col)) return fail(MI_EINVAL, "NULL argument");
    if (kind != MI_KIND_CSR_RANK1 && kind != MI_KIND_POTTS_CSR) return fail(MI_EINVAL, "the structured kinds only (got %d)", kind);
    if (R < 1) return fail(MI_EINVAL, "R must be >= 1 (got %d)", R);
    return guarded([&]() -> int {
        std::string err;
        SlotModelFacts facts;
        int rc = slot_model_size_check(kind, n, kind == MI_KIND_CSR_RANK1 ? 2 : K, &err);
        if (!rc) rc = slot_model_facts(kind, rowptr, col, n, kind == MI_KIND_CSR_RANK1 ? 2 : K, getenv("MI_K2_STATE"), &facts, &err);
        if (rc) return fail(rc, "%s", err.c_str());
        PlanOptions opts;
        MI_TRY(parse_option_string(options, [&](const char *key, long value) { return plan_option_set(opts, key, value); }));
        RunFacts run;
        run.R = R; run.cus = cus; run.pair_weight_slot = kind == MI_KIND_CSR_RANK1 ? pair_weight_slot : -1;
        run.node_weights = node_weights != 0; run.min_cluster_size = min_cluster_size;
        AnnealPlan plan;
        if ((rc = plan_anneal(facts, run, opts, &plan, &err))) return fail(rc, "%s", err.c_str());
        plan_kernel_name(plan, out_kernel, (size_t)len);
        if (out_adjacency_bytes) *out_adjacency_bytes = plan.adj_bytes;
        return MI_OK;
    });
}

int mi_sa_problem_create_csr_rank1_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                       const float *lin, float c_pair, int n, double offset, int device,
                                       mi_sa_problem **out)
{
    return guarded([&]() -> int {
        if (!rowptr || !lin || !out || (rowptr[n > 0 ? n : 0] > 0 && (!col || !val))) return fail(MI_EINVAL, "NULL argument");
        std::string err;
        if (const int rc_s = slot_model_size_check(MI_KIND_CSR_RANK1, n, 2, &err)) return fail(rc_s, "%s", err.c_str());
        return new_problem(MI_KIND_CSR_RANK1, n, 2, offset, 1, device, out, [&](mi_sa_problem *p) -> int {
            p->slot.c_pair = c_pair;
            MI_TRY(upload_slot_ell(p, rowptr, col, val, n));
            return upload_linear_terms(p, lin);
        });
    });
}

int mi_sa_problem_create_potts_csr_f32(const int32_t *rowptr, const int32_t *col, const float *val,
                                       float c_pair, int n, int K, double lin_offset, int device,
                                       mi_sa_problem **out)
{
    return guarded([&]() -> int {
        if (!rowptr || !out || (rowptr[n > 0 ? n : 0] > 0 && (!col || !val))) return fail(MI_EINVAL, "NULL argument");
        std::string err;
        if (const int rc_s = slot_model_size_check(MI_KIND_POTTS_CSR, n, K, &err)) return fail(rc_s, "%s", err.c_str());
        return new_problem(MI_KIND_POTTS_CSR, n, K, lin_offset, 2, device, out, [&](mi_sa_problem *p) -> int {
            p->slot.c_pair = c_pair;
            for (int e = 0; e < rowptr[n]; ++e) p->merge.sumabs += std::fabs((double)val[e]);   // (sequential, in stored order)
            return upload_slot_ell(p, rowptr, col, val, n);
        });
    });
}

int mi_sa_problem_set_energy_model_f64(mi_sa_problem *p, const double *val, const double *lin, double c_pair)
{
    return on_problem(p, NO_ARGS, STREAM_IDLE, [&]() -> int {
        mi_sa_problem::Slot &m = p->slot;
        if (p->kind != MI_KIND_CSR_RANK1 && p->kind != MI_KIND_POTTS_CSR)
            return fail(MI_EUNSUPPORTED, "an fp64 energy model is defined for the structured kinds only");
        const int n = p->n, D = m.D;
        const int64_t nnz = m.h_rowptr.empty() ? 0 : m.h_rowptr[n];
        if ((nnz > 0 && !val) || (p->kind == MI_KIND_CSR_RANK1 && !lin)) return fail(MI_EINVAL, "NULL argument");
        std::vector<double> hv((size_t)m.slots * D * 64, 0.0), hl((size_t)m.slots * 64, 0.0);
        for (int i = 0; i < n; ++i) {
            const int t = i >> 6, lane = i & 63;
            for (int e = m.h_rowptr[i], k = 0; e < m.h_rowptr[i + 1]; ++e, ++k) hv[((size_t)t * D + k) * 64 + lane] = val[e];
            if (lin) hl[i] = lin[i];
        }
        HIP_TRY(m.d_ell_val64.upload(hv));
        HIP_TRY(m.d_lin64.upload(hl));
        m.c_pair64 = c_pair;
        return MI_OK;
    });
}

int mi_sa_problem_set_absent(mi_sa_problem *p, const uint8_t *absent)
{
    return on_problem(p, absent != nullptr, STREAM_IDLE, [&]() -> int {
        std::vector<uint32_t> &h_meta = p->slot.h_meta;
        if (p->kind != MI_KIND_POTTS_CSR)
            return fail(MI_EUNSUPPORTED, "holes of a Potts model only (a binary CSR model marks them by lin = +inf)");
        for (int i = 0; i < p->n; ++i) {
            if (absent[i] && (h_meta[(size_t)i] & 0x00ffff00u))
                return fail(MI_EINVAL, "variable %d is marked absent but has couplings", i);
            h_meta[(size_t)i] = (h_meta[(size_t)i] & 0x7fffffffu) | (absent[i] ? 0x80000000u : 0u);
        }
        HIP_TRY(p->slot.d_meta.upload(h_meta));
        return MI_OK;
    });
}

int mi_sa_problem_set_pair_weights(mi_sa_problem *p, const int32_t *weights)
{
    return on_problem(p, weights != nullptr, STREAM_IDLE, [&]() -> int {
        const mi_sa_problem::Slot &m = p->slot;
        if (p->kind != MI_KIND_CSR_RANK1)
            return fail(MI_EUNSUPPORTED, "pair-term weights: structured binary (CSR + uniform pair) problems only");
        int wslot = -1;
        for (int i = 0; i < p->n; ++i) {
            if (m.h_meta[(size_t)i] >> 31) continue;          // (never set for this kind; holes are marked by lin = +inf)
            const bool hole = !m.h_hole.empty() && m.h_hole[(size_t)i];
            if (hole) continue;
            if (weights[i] < 1) return fail(MI_EINVAL, "weight %d of variable %d: weights are positive integers", weights[i], i);
            if (weights[i] > (1 << 20)) return fail(MI_EINVAL, "weight %d of variable %d exceeds 2^20", weights[i], i);
            if (weights[i] == 1) continue;
            if (m.h_rowptr[(size_t)i + 1] != m.h_rowptr[(size_t)i])
                return fail(MI_EINVAL, "variable %d has weight %d and sparse couplings: weighted variables couple through the pair term only", i, weights[i]);
            if (wslot >= 0 && wslot != i / 64)
                return fail(MI_EINVAL, "variables with weights other than 1 in slots %d and %d: they must share one 64-variable slot", wslot, i / 64);
            wslot = i / 64;
        }
        std::vector<int32_t> hw(64, 0);
        if (wslot >= 0) {
            for (int l = 0; l < 64; ++l) {
                const int i = wslot * 64 + l;
                if (i >= p->n || (!m.h_hole.empty() && m.h_hole[(size_t)i])) continue;
                hw[(size_t)l] = weights[i];
            }
            // a variable of weight 1 may share the slot (it is swept by the same serial loop) -- but it must have no sparse
            // couplings either: the loop does not update neighbours
            for (int l = 0; l < 64; ++l) {
                const int i = wslot * 64 + l;
                if (i < p->n && hw[(size_t)l] != 0 && m.h_rowptr[(size_t)i + 1] != m.h_rowptr[(size_t)i])
                    return fail(MI_EINVAL, "variable %d shares the weighted slot %d and has sparse couplings", i, wslot);
            }
        }
        HIP_TRY(p->slot.d_wgt.upload(hw));
        p->slot.wslot = wslot;
        return MI_OK;
    });
}

int mi_sa_problem_set_node_weights(mi_sa_problem *p, const int32_t *wq, const float *cw, const double *w64)
{
    return on_problem(p, wq && cw, STREAM_IDLE, [&]() -> int {
        if (p->kind != MI_KIND_POTTS_CSR) return fail(MI_EINVAL, "node weights: Potts problems only");
        if (p->last.has_run) return fail(MI_EINVAL, "node weights must be set before the first anneal");
        if (p->opt.min_cluster_size > 0) return fail(MI_EUNSUPPORTED, "node weights together with min_cluster_size are not supported");
        const size_t seats = (size_t)p->slot.slots * 64;
        std::vector<int32_t> hq(seats, 0);
        std::vector<float> hc(seats, 0.0f);
        std::vector<double> hw(seats, 0.0);
        int64_t total = 0;
        for (int i = 0; i < p->n; ++i) {
            if (p->slot.h_meta[(size_t)i] >> 31) continue;             // a hole: weight 0, in no cluster
            if (wq[i] < 0 || (w64 && !(w64[i] >= 0.0)))
                return fail(MI_EINVAL, "weight of variable %d is negative", i);
            total += wq[i];
            if (total > (int64_t)1 << 30) return fail(MI_EINVAL, "the node weights sum to more than 2^30");
            hq[(size_t)i] = wq[i];
            hc[(size_t)i] = cw[i];
            hw[(size_t)i] = w64 ? w64[i] : (double)wq[i];
        }
        // (d_ncw may already hold ngroups x seats coefficients: the first group's are rewritten)
        HIP_TRY(p->nw.d_nwq.upload(hq));
        HIP_TRY(p->nw.d_ncw.reserve(seats));
        HIP_TRY(hipMemcpy(p->nw.d_ncw, hc.data(), seats * sizeof(float), hipMemcpyHostToDevice));
        HIP_TRY(p->nw.d_nw64.upload(hw));
        return MI_OK;
    });
}

int mi_sa_problem_set_node_weight_groups(mi_sa_problem *p, int G, const float *cw, const double *c64, const double *offset)
{
    return on_problem(p, cw && c64 && offset, STREAM_IDLE, [&]() -> int {
        if (G < 1 || G > 256) return fail(MI_EINVAL, "resolution groups: 1 .. 256 (got %d)", G);
        if (!p->nw.d_nwq) return fail(MI_EINVAL, "resolution groups need node weights (mi_sa_problem_set_node_weights) first");
        if (p->last.has_run) return fail(MI_EINVAL, "resolution groups must be set before the first anneal");
        const size_t seats = (size_t)p->slot.slots * 64;
        std::vector<float> hc((size_t)G * seats, 0.0f);
        for (int g = 0; g < G; ++g) {
            for (int i = 0; i < p->n; ++i)
                if (!(p->slot.h_meta[(size_t)i] >> 31)) hc[(size_t)g * seats + i] = cw[(size_t)g * p->n + i];   // (holes: 0)
        }
        std::vector<double> hk(c64, c64 + G);
        hk.insert(hk.end(), offset, offset + G);
        // the coefficients go into an array of their own, which takes the place of d_ncw once everything has succeeded:
        // a failure leaves the problem as it was
        DevArray<float> ncw;
        HIP_TRY(ncw.upload(hc));
        HIP_TRY(p->nw.d_gconst.reserve(2 * 256));
        HIP_TRY(hipMemcpy(p->nw.d_gconst, hk.data(), hk.size() * sizeof(double), hipMemcpyHostToDevice));
        p->nw.d_ncw.swap(ncw);
        p->nw.ngroups = G;
        return MI_OK;
    });
}

// chain 2e: the exponent f of the fixed-point couplings vq = llrint(S_uv 2^f), the largest with sum |S_uv| 2^f <= 2^62
// (clamped to [-1000, 1000]; 0 without couplings)
static int merge_fixed_exponent(double sumabs)
{
    if (!(sumabs > 0.0)) return 0;
    int E = 0;
    const double m = std::frexp(sumabs, &E);              // sumabs = m 2^E, m in [1/2, 1)
    const int f = 62 - E + (m == 0.5 ? 1 : 0);
    return f < -1000 ? -1000 : (f > 1000 ? 1000 : f);
}

int mi_sa_problem_set_merge_moves(mi_sa_problem *p, int interval, int proposals, const double *cq)
{
    return on_problem(p, NO_ARGS, 0, [&]() -> int {
        if (p->kind != MI_KIND_POTTS_CSR) return fail(MI_EINVAL, "merge moves: Potts problems only");
        if (interval < 0) return fail(MI_EINVAL, "merge interval must be >= 0 (got %d)", interval);
        if (proposals < 1) return fail(MI_EINVAL, "merge proposals must be >= 1 (got %d)", proposals);
        if (interval == 0) { p->merge.interval = 0; return MI_OK; }
        if (p->K < 2) return fail(MI_EINVAL, "merge moves need K >= 2");
        if (p->nw.d_nwq && !cq) return fail(MI_EINVAL, "merge moves on a problem with node weights need the coefficients cq");
        if (p->opt.min_cluster_size > 0) return fail(MI_EUNSUPPORTED, "merge moves together with min_cluster_size are not supported");
        if (p->pt.T > 0) return fail(MI_EUNSUPPORTED, "merge moves under tempering are not supported");
        const int G = p->nw.ngroups;
        std::vector<double> h((size_t)G, (double)p->slot.c_pair);
        if (cq)
            for (int g = 0; g < G; ++g) {
                if (!std::isfinite(cq[g])) return fail(MI_EINVAL, "cq[%d] is not finite", g);
                h[(size_t)g] = cq[g];
            }
        HIP_TRY(hipSetDevice(p->device));        // (not on the way in: switching the moves off touches no device)
        HIP_TRY(hipStreamSynchronize(p->stream));
        HIP_TRY(p->merge.d_cq.reserve(256));
        HIP_TRY(hipMemcpy(p->merge.d_cq, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        p->merge.cq = cq ? h : std::vector<double>();
        p->merge.interval = interval;
        p->merge.proposals = proposals;
        return MI_OK;
    });
}

// what needs the handle alive: the worker joined, the device current, the stream idle; the members release the rest
int mi_sa_problem_destroy(mi_sa_problem *p)
{
    if (!p) return MI_OK;
    (void)guarded([&]() -> int { return settle(p); });
    (void)hipSetDevice(p->device);
    if (p->stream) (void)hipStreamSynchronize(p->stream);
    delete p;
    return MI_OK;
}

int mi_sa_problem_info(const mi_sa_problem *p, int *kind, int *n, int *num_cases, int *device)
{
    if (!p) return guarded([]() -> int { return fail(MI_EINVAL, "NULL problem"); });
    if (kind) *kind = p->kind;
    if (n) *n = p->n;
    if (num_cases) *num_cases = p->K;
    if (device) *device = p->device;
    return MI_OK;
}

int mi_sa_debug_stats(mi_sa_problem *p, uint64_t *out, int words)
{
    return on_problem(p, out != nullptr, STREAM_IDLE, [&]() -> int {
        if (words > 16) words = 16;
        HIP_TRY(hipMemcpy(out, p->run.d_stats, (size_t)words * sizeof(uint64_t), hipMemcpyDeviceToHost));
        if (words == 16 && p->dense.d_ctrl) {                   // [14], [15]: chunks of the last scheduled dense run served by K1w / K1m
            unsigned int c[2] = {0, 0};
            HIP_TRY(hipMemcpy(c, p->dense.d_ctrl + 4, sizeof c, hipMemcpyDeviceToHost));
            out[14] = c[0]; out[15] = c[1];
        }
        return MI_OK;
    });
}

int mi_sa_debug_pace(mi_sa_problem *p, unsigned int *out, int words)
{
    return on_problem(p, out != nullptr, STREAM_IDLE, [&]() -> int {
        if (words > kPaceWords) words = kPaceWords;
        HIP_TRY(hipMemcpy(out, p->run.d_pace, (size_t)words * sizeof(unsigned int), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_sa_set_option(mi_sa_problem *p, const char *key, long value)
{
    return on_problem(p, key != nullptr, 0, [&]() -> int {
        mi_sa_problem::Options &o = p->opt;
        if (dense_plan_option_set(o.dense, key, value)) return MI_OK;      // (pace, variant, unit_rows, chunk_sweeps, *_permille: csrc/mi_dense_plan.h)
        if (!strcmp(key, "xl_batched") && value >= 0 && value <= 2) { o.xl_batched = (int)value; return MI_OK; }
        if (!strcmp(key, "xl_chunk") && value >= 1) { o.xl_chunk = (int)value; return MI_OK; }
        if (!strcmp(key, "xl_chain") && value >= 0 && value <= 2) { o.xl_chain = (int)value; return MI_OK; }
        if (!strcmp(key, "xl_cold_permille") && value >= 0 && value <= 1000) { o.xl_cold_permille = (int)value; return MI_OK; }
        if (!strcmp(key, "xl_async") && value >= 0 && value <= 1) { o.xl_async = (int)value; return MI_OK; }
        if (!strcmp(key, "debug")) { o.debug = (int)value; return MI_OK; }
        if (plan_option_set(o.plan, key, value)) return MI_OK;             // (the k2_* / k3_* keys: csrc/mi_sa_plan.h)
        if (!strcmp(key, "min_cluster_size") && value >= 0) {
            if (p->kind != MI_KIND_POTTS_CSR) return fail(MI_EINVAL, "min_cluster_size applies to Potts problems");
            if (value > 0 && p->nw.d_nwq) return fail(MI_EUNSUPPORTED, "min_cluster_size together with node weights is not supported");
            if (value > 0 && p->merge.interval > 0) return fail(MI_EUNSUPPORTED, "min_cluster_size together with merge moves is not supported");
            o.min_cluster_size = (int)value;
            return MI_OK;
        }
        return fail(MI_EINVAL, "unknown option '%s'", key);
    });
}

}  // extern "C"

// ---- one anneal: its arguments decoded and staged, then the arm of the problem's kind -------------------------------
namespace {

struct AnnealCall {
    int R, num_sweeps, resync, G;                // G: resolution groups (1 unless mi_sa_problem_set_node_weight_groups)
    uint32_t replica_offset, sweep_offset, seed_lo, seed_hi;
    bool per_replica, per_group, merges;
    const void *host_init;                       // the caller's initial states (null: none)
    const float *temps;                          // device: the temperatures of the run
    const void *init;                            // device: where the chains start (null: from their random words)
    void *states;
};

// the fields DenseXlArgs, DenseArgs and EllArgs share
template <typename Args>
void fill_common(Args &a, const mi_sa_problem *p, const AnnealCall &c)
{
    a.temps = c.temps;
    a.init = static_cast<decltype(a.init)>(c.init);
    a.states = static_cast<decltype(a.states)>(c.states);
    a.energy = p->run.d_energy; a.stats = p->run.d_stats;
    a.offset = p->offset; a.n = p->n; a.R = c.R; a.num_sweeps = c.num_sweeps; a.resync = c.resync;
    a.replica_offset = c.replica_offset; a.seed_lo = c.seed_lo; a.seed_hi = c.seed_hi;
    a.sweep_offset = c.sweep_offset; a.temps_per_replica = c.per_replica ? 1 : 0;
}

// validates the arguments of an anneal, sizes the run buffers, uploads temperatures and initial states, resets the
// statistics and leaves the inputs resident before the timed region
int stage_anneal(mi_sa_problem *p, int R, uint32_t replica_offset, int num_sweeps, const double *betas, uint64_t seed,
                 const void *init, int resync_interval, uint32_t sweep_offset, uint32_t flags, AnnealCall *c)
{
    const bool cont = (flags & MI_F_CONTINUE) != 0, resident = (flags & MI_F_TEMPS_RESIDENT) != 0;
    const bool per_replica = (flags & MI_F_BETA_PER_REPLICA) != 0 || resident;
    const bool per_group = (flags & MI_F_BETA_PER_GROUP) != 0;
    if (flags & ~(uint32_t)(MI_F_CONTINUE | MI_F_BETA_PER_REPLICA | MI_F_TEMPS_RESIDENT | MI_F_BETA_PER_GROUP))
        return fail(MI_EINVAL, "unknown flags 0x%x", flags);
    const int G = p->nw.ngroups;
    if (per_group && per_replica) return fail(MI_EINVAL, "MI_F_BETA_PER_GROUP together with per-replica temperatures");
    if (G > 1 && per_replica)
        return fail(MI_EUNSUPPORTED, "resolution groups together with per-replica or resident temperatures are not supported");
    if (R % G != 0) return fail(MI_EINVAL, "R = %d is not a multiple of the %d resolution groups", R, G);
    const int num_betas = per_replica ? R : (per_group ? G * num_sweeps : num_sweeps);
    if (resident && (p->pt.T == 0 || p->pt.R_local != R))
        return fail(MI_ESTATE, "MI_F_TEMPS_RESIDENT needs mi_sa_tempering_begin for %d replicas on this problem", R);
    if (R < 1) return fail(MI_EINVAL, "R must be >= 1 (got %d)", R);
    if (num_sweeps < 0) return fail(MI_EINVAL, "num_sweeps must be >= 0");
    if (num_betas > 0 && num_sweeps > 0 && !betas && !resident) return fail(MI_EINVAL, "betas is NULL");
    if (cont && (!p->last.has_run || p->last.R != R))
        return fail(MI_ESTATE, "MI_F_CONTINUE needs a previous run with the same number of replicas");
    if (cont && init) return fail(MI_EINVAL, "MI_F_CONTINUE and init are mutually exclusive");
    if (resync_interval < 0) return fail(MI_EINVAL, "resync_interval must be >= 0");
    const bool merges = p->kind == MI_KIND_POTTS_CSR && p->merge.interval > 0 && num_sweeps > 0;
    if (merges && resident) return fail(MI_EUNSUPPORTED, "merge moves with resident (tempering) temperatures are not supported");
    if (merges && p->nw.d_nwq && p->merge.cq.empty())
        return fail(MI_EINVAL, "merge moves on a problem with node weights need the coefficients cq");
    if (merges && !p->merge.cq.empty() && p->merge.cq.size() != (size_t)G)
        return fail(MI_EINVAL, "merge moves: %zu coefficients for %d resolution groups", p->merge.cq.size(), G);
    for (int s = 0; s < (num_sweeps > 0 && !resident ? num_betas : 0); ++s)
        if (!(betas[s] > 0.0) || !std::isfinite(betas[s]))
            return fail(MI_EINVAL, "betas[%d] = %g is not a positive finite number", s, betas[s]);
    // (the device buffer of the temperatures holds G x num_sweeps values: one schedule per group, or one shared)
    MI_TRY(ensure_run_buffers(p, R, G * num_sweeps > num_betas ? G * num_sweeps : num_betas, init != nullptr));
    mi_sa_problem::Run &b = p->run;
    if (!resident) {                             // (tempering rounds: the exchange kernel keeps temps[] up to date)
        std::vector<float> temps((size_t)(num_betas > 0 ? num_betas : 1), 1.0f);
        for (int s = 0; s < (num_sweeps > 0 ? num_betas : 0); ++s) temps[s] = (float)(1.0 / betas[s]);
        // pageable-host async copies are staged synchronously by the runtime: the vector may go away
        HIP_TRY(hipMemcpyAsync(b.d_temps, temps.data(), temps.size() * sizeof(float), hipMemcpyHostToDevice, p->stream));
    }
    if (init)
        HIP_TRY(hipMemcpyAsync(b.d_init, init, (size_t)R * p->n * p->state_elem, hipMemcpyHostToDevice, p->stream));
    HIP_TRY(hipMemsetAsync(b.d_stats, 0, 16 * sizeof(unsigned long long), p->stream));
    if (!resident || init)
        HIP_TRY(hipStreamSynchronize(p->stream));   // inputs resident before the timed region
    g_kernel.clear();
    p->last.adj_bytes = 0;
    p->last.launches = 1;
    *c = AnnealCall{R, num_sweeps, resync_interval, G, replica_offset, sweep_offset, (uint32_t)seed, (uint32_t)(seed >> 32),
                    per_replica, per_group, merges, init, resident ? p->pt.d_temps.p : b.d_temps.p,
                    cont ? b.d_states.p : (init ? b.d_init.p : nullptr), b.d_states.p};
    return MI_OK;
}

// the run of a dense anneal as the planners see it (csrc/mi_dense_plan.h)
DenseRun dense_run_of(const mi_sa_problem *p, const AnnealCall &call)
{
    DenseRun run;
    run.n = p->n; run.R = call.R; run.num_sweeps = call.num_sweeps; run.resync = call.resync;
    run.temps_per_replica = call.per_replica; run.cus = p->cus; run.resident_waves = p->dense.resident_waves;
    return run;
}

int anneal_dense_xl(mi_sa_problem *p, const AnnealCall &call)
{
    const mi_sa_problem::Options &o = p->opt;
    const int R = call.R, num_sweeps = call.num_sweeps;
    DenseXlArgs a;
    fill_common(a, p, call);
    a.Q2 = p->xl.d_Q2; a.diag = p->xl.d_diag;
    a.xg_chain = o.xl_chain;
    // K1x pays per accepted flip (a barrier and the L2 latency of one Q row: ~1 us up to n = 8192, 3 us at 20 000,
    // 8 us at 50 000) and runs 256 replicas at a time; K1g pays ~25 us per 64 rows whatever the replica count
    // below 256.  Measured (profiles/r02_xl_crossover.json): K1x wins at n <= 8192 with <= 64 replicas (2-3x),
    // K1g from n = 20 000 at any count (1.1-2x over a whole schedule, 9x on its hot part at 50 000).
    const bool batched = o.xl_batched == 1 || (o.xl_batched == 0 && (R >= 256 || p->n >= 16384));
    if (batched) HIP_TRY(p->xl.d_xg.reserve(mi_dense_xg_workspace_bytes(p->n, R)));
    HIP_TRY(hipEventRecord(p->ev.e[0], p->stream));
    if (!batched) {
        MI_TRY(mi_launch_dense_xl(a, p->xl.chunks, p->stream));
    } else if (call.resync > 0 || call.per_replica || num_sweeps <= o.xl_chunk || o.xl_cold_permille == 0) {
        MI_TRY(mi_launch_dense_xg(a, p->xl.chunks, p->xl.d_xg, p->stream, 3));
    } else {
        // K1g costs the same hot or cold (two launches per 64 rows whether anything flips or not); K1x costs per
        // accepted flip.  Along a cooling schedule: K1g in chunks of sweeps while the chunks accept enough, then
        // K1x for the rest, continuing from K1g's states AND cached fields (same chain, bit for bit).  The hand-over
        // is decided on the host, chunk by chunk -- a device-side mode word as on the n <= 4096 scheduler would need
        // every chunk's launches enqueued in advance (1600 per sweep at n = 50 000, each an empty launch once the
        // run has gone cold: seconds) -- so a worker thread of the problem waits for the chunks and this call
        // returns at once, like every other anneal; the next call on the problem joins it (settle).
        auto cooling_run = [p, a, num_sweeps, R]() -> int {
            HIP_TRY(hipSetDevice(p->device));
            const mi_sa_problem::Options &o = p->opt;
            unsigned long long *accepted = p->run.d_stats + 1;
            int s0 = 0;
            while (s0 < num_sweeps) {
                const int len = num_sweeps - s0 < o.xl_chunk ? num_sweeps - s0 : o.xl_chunk;
                DenseXlArgs b = a;
                b.num_sweeps = len; b.temps = a.temps + s0; b.sweep_offset = a.sweep_offset + (uint32_t)s0;
                unsigned long long before = 0, after = 0;
                HIP_TRY(hipMemcpyAsync(&before, accepted, sizeof before, hipMemcpyDeviceToHost, p->stream));
                MI_TRY(mi_launch_dense_xg(b, p->xl.chunks, p->xl.d_xg, p->stream, (s0 == 0 ? 1 : 0) | 2));
                s0 += len;
                if (s0 >= num_sweeps) break;
                HIP_TRY(hipMemcpyAsync(&after, accepted, sizeof after, hipMemcpyDeviceToHost, p->stream));
                HIP_TRY(hipStreamSynchronize(p->stream));
                const double share = (double)(after - before) / ((double)R * (double)p->n * (double)len);
                if (share * 1000.0 < (double)o.xl_cold_permille) {
                    DenseXlArgs c = a;
                    c.num_sweeps = num_sweeps - s0; c.temps = a.temps + s0; c.sweep_offset = a.sweep_offset + (uint32_t)s0;
                    c.init = a.states;                                 // written by the chunk that just ended
                    c.fields_in = mi_dense_xg_fields(p->xl.d_xg);
                    c.fin_ncols = (p->n + 255) / 256 * 256;
                    MI_TRY(mi_launch_dense_xl(c, p->xl.chunks, p->stream));
                    break;
                }
            }
            HIP_TRY(hipEventRecord(p->ev.e[1], p->stream));
            return MI_OK;
        };
        if (!o.xl_async) return cooling_run();
        // (no exception leaves the thread: one of the run, or of keeping its texts, becomes the worker's error)
        p->xl.worker = std::thread([p, cooling_run]() {
            g_kernel.clear(); g_err.clear();
            p->xl.worker_rc = guarded([&]() -> int {
                const int rc = guarded(cooling_run);
                p->xl.worker_err = g_err;
                p->xl.worker_kernel = g_kernel;
                return rc;
            });
        });
        return MI_OK;
    }
    HIP_TRY(hipEventRecord(p->ev.e[1], p->stream));
    return MI_OK;
}

// sweeps until the first field re-synchronisation of a launch that starts at sweep s0 of its run
inline int resync_first_for(int resync, int s0)
{
    return resync > 0 ? ((resync - s0 % resync) % resync) + 1 : 0;
}

// n <= 4096: the plan says which kernel(s), on which sweeps and replicas, with which buffers (csrc/mi_dense_plan.h); this
// walks its launches.  A run that is cut keeps its state (DenseArgs::states) and cached fields (DenseArgs::fields) in HBM
// between launches, so the cut points are invisible to the chain -- results are bit-identical to one launch.
int anneal_dense(mi_sa_problem *p, const AnnealCall &call)
{
    mi_sa_problem::Dense &d = p->dense;
    const DenseWidth unit = dense_width_unit(d.NT);
    if (!unit.launch) return fail(MI_EUNSUPPORTED, "dense kernel not built for NT=%d", d.NT);
    if (!d.resident_waves && dense_plan_is_k1(dense_run_of(p, call), p->opt.dense)) {     // K1's occupancy at this width: asked once, by the first run K1 serves
        int blocks_per_cu = 0;
        MI_TRY(unit.k1_blocks_per_cu(&blocks_per_cu));
        d.resident_waves = blocks_per_cu * p->cus * 4;
    }
    DensePlan plan;
    std::string plan_err;
    if (const int rc_p = plan_dense(dense_run_of(p, call), p->opt.dense, &plan, &plan_err)) return fail(rc_p, "%s", plan_err.c_str());
    if (plan.field_floats) HIP_TRY(d.d_fields.reserve(plan.field_floats));
    if (plan.form == DENSE_SCHEDULED && !d.d_ctrl) HIP_TRY(d.d_ctrl.resize(kCtrlWords));
    char name[128];
    dense_plan_kernel_name(plan, name, sizeof name);
    note_kernel("%s", name);
    p->last.launches = plan.launches;

    DenseArgs a;
    fill_common(a, p, call);
    a.Qp = d.d_Qp; a.Qm = d.d_Qm; a.pace = nullptr;
    a.debug = p->opt.debug; a.ondemand_flips = 0;
    a.fields = nullptr; a.ctrl = nullptr; a.flags = 0; a.my_mode = 0; a.mode_up_flips = 0; a.chunk_index = 0;
    a.resync_first = resync_first_for(a.resync, 0);
    unsigned int *d_pace = p->run.d_pace;
    hipStream_t st = p->stream;
    HIP_TRY(hipEventRecord(p->ev.e[0], st));
    if (plan.form == DENSE_K1) {
        // launches of at most `resident` replicas (= wavefronts), so that every wave of a launch is co-resident and the sweep
        // pacing rendezvous can complete; they run back to back on the stream, each with its own zeroed pacing words
        if (plan.k1_pace) HIP_TRY(hipMemsetAsync(d_pace, 0, kMaxChunks * kPaceWords * sizeof(unsigned int), st));
        for (int lo = 0, c = 0; lo < call.R; lo += plan.replicas_per_launch, ++c) {
            DenseArgs b = a;
            b.R = call.R - lo < plan.replicas_per_launch ? call.R - lo : plan.replicas_per_launch;
            b.replica_offset = a.replica_offset + (uint32_t)lo;
            b.init = a.init ? a.init + (size_t)lo * a.n : nullptr;
            b.states = a.states + (size_t)lo * a.n;
            b.energy = a.energy + lo;
            b.temps = a.temps + (a.temps_per_replica ? lo : 0);          // one temperature per replica: the launch's own
            b.pace = dense_k1_paced(plan, b.R) ? d_pace + (size_t)c * kPaceWords : nullptr;
            MI_TRY(unit.launch(b, 0, st));
        }
    } else {
        auto launch_k1w = [&](DenseArgs b) -> int {
            b.ondemand_flips = plan.ondemand_flips;
            if (plan.wg_pace && b.num_sweeps > 1) {
                HIP_TRY(hipMemsetAsync(d_pace, 0, kPaceWords * sizeof(unsigned int), st));
                b.pace = d_pace;
            }
            return unit.launch(b, plan.unit_rows, st);
        };
        if (plan.form == DENSE_SCHEDULED) {
            // every launch is offered to both kernels, the device-side mode word decides
            HIP_TRY(hipMemsetAsync(d.d_ctrl, 0, kCtrlWords * sizeof(unsigned int), st));
            const unsigned int start = kModeMfma;            // start hot; a short first launch calibrates
            HIP_TRY(hipMemcpyAsync(d.d_ctrl + kCtrlModes, &start, sizeof start, hipMemcpyHostToDevice, st));
        }
        for (int i = 0; i < plan.steps; ++i) {
            const DenseStep step = dense_plan_step(plan, i);
            DenseArgs b = a;
            b.num_sweeps = step.len;
            b.temps = a.temps_per_replica ? a.temps : a.temps + step.s0;
            b.sweep_offset = a.sweep_offset + (uint32_t)step.s0;
            b.init = step.first ? a.init : a.states;
            b.resync_first = resync_first_for(a.resync, step.s0);
            b.chunk_index = i;
            if (plan.cut) {
                b.fields = d.d_fields;
                b.flags = (step.first ? 0 : kDenseFieldsIn) | (step.last ? 0 : (kDenseFieldsOut | kDenseNoEnergy));
            }
            if (plan.form == DENSE_SCHEDULED) {
                // next launch goes to K1m when this one accepted at least mfma_permille of its proposals
                b.ctrl = d.d_ctrl;
                b.mode_up_flips = (unsigned int)((double)p->opt.dense.mfma_permille * 1e-3 * (double)a.R * a.n * b.num_sweeps);
                if (b.mode_up_flips == 0) b.mode_up_flips = 1;
                b.my_mode = (int)kModeMfma;
                MI_TRY(unit.launch_mfma(b, st));
                b.my_mode = (int)kModeWg;
                MI_TRY(launch_k1w(b));
            } else {
                MI_TRY(plan.form == DENSE_K1M ? unit.launch_mfma(b, st) : launch_k1w(b));
            }
        }
    }
    HIP_TRY(hipEventRecord(p->ev.e[1], st));
    return MI_OK;
}

// the kernel of a structured anneal is the plan's to say (csrc/mi_sa_plan.h); the launchers only find its instantiation
int launch_structured(const AnnealPlan &plan, const EllArgs &b, hipStream_t st)
{
    switch (plan.family) {
    case PLAN_K2P: return mi_launch_csr_rank1_pair(b, plan, st);
    case PLAN_K2W: case PLAN_K2S: return mi_launch_csr_rank1_split(b, plan, st);
    case PLAN_K3F: return mi_launch_potts_fast(b, plan, st);
    default: return mi_launch_sparse(b, plan, st);
    }
}

// chain 2e: a merge phase before every global sweep s > 0 with s % M == 0 inside this call; the anneal launches between
// them continue from the labels in HBM, as MI_F_CONTINUE does
int anneal_potts_with_merges(mi_sa_problem *p, const AnnealCall &call, const EllArgs &a, const AnnealPlan &plan)
{
    MergeArgs m;
    m.ell_col = a.ell_col; m.ell_val = a.ell_val; m.meta = a.meta; m.nwq = a.nwq;
    m.cq = p->merge.d_cq; m.temps = a.temps; m.temps_per_replica = a.temps_per_replica;
    m.temps_group_stride = a.temps_group_stride; m.states = static_cast<uint16_t *>(a.states);
    m.stats = a.stats;
    const int f = merge_fixed_exponent(p->merge.sumabs);
    m.scale = std::ldexp(1.0, f); m.inv_scale = std::ldexp(1.0, -f);
    m.n = a.n; m.K = a.K; m.R = a.R; m.D = a.D; m.groups = a.groups; m.proposals = p->merge.proposals;
    m.replica_offset = a.replica_offset; m.seed_lo = a.seed_lo; m.seed_hi = a.seed_hi;
    const uint32_t M = (uint32_t)p->merge.interval;
    const void *labels = a.init;          // where the next launch finds the labels (null: tag-1 words)
    int launches = 0, merge_launches = 0;
    for (int s0 = 0; s0 < call.num_sweeps;) {
        const uint32_t s = call.sweep_offset + (uint32_t)s0;
        if (s > 0 && s % M == 0) {
            m.src = static_cast<const uint16_t *>(labels); m.sweep = s; m.sweep_local = s0;
            MI_TRY(mi_launch_potts_merge(m, p->stream));
            labels = a.states;
            ++launches; ++merge_launches;
        }
        const int len = (int)std::min<uint32_t>((uint32_t)(call.num_sweeps - s0), M - s % M);
        EllArgs b = a;
        b.init = labels; b.num_sweeps = len; b.sweep_offset = s;
        if (!call.per_replica) b.temps = a.temps + s0;   // (per group: + g * temps_group_stride inside the kernel)
        MI_TRY(launch_structured(plan, b, p->stream));
        labels = a.states;
        ++launches;
        s0 += len;
    }
    if (merge_launches) note_kernel("k_potts_merge");
    p->last.launches = launches;
    return MI_OK;
}

int anneal_structured(mi_sa_problem *p, const AnnealCall &call)
{
    const mi_sa_problem::Slot &m = p->slot;
    EllArgs a;
    fill_common(a, p, call);
    a.ell_col = m.d_ell_col; a.ell_val = m.d_ell_val; a.lin = m.d_lin;
    a.c_pair = m.c_pair; a.K = p->K; a.slots = m.slots; a.D = m.D;
    a.rows = m.d_rows; a.meta = m.d_meta; a.slot_flags = m.d_slot_flags; a.state_bytes = m.facts.state_bytes;
    a.waves_override = p->opt.plan.k2_waves; a.min_size = p->opt.min_cluster_size;
    a.ell_val64 = m.d_ell_val64; a.lin64 = m.d_lin64; a.c_pair64 = m.c_pair64;
    a.wgt = m.d_wgt; a.wslot = p->kind == MI_KIND_CSR_RANK1 ? m.wslot : -1;
    a.nwq = p->nw.d_nwq; a.ncw = p->nw.d_ncw; a.nw64 = p->nw.d_nw64;
    a.groups = call.G; a.temps_group_stride = call.per_group ? call.num_sweeps : 0; a.gconst = p->nw.d_gconst;
    if (p->kind == MI_KIND_POTTS_CSR && call.host_init) {
        // labels must be < K: validated on the host copy (the device trusts them as cnt[] indices)
        const uint16_t *l = static_cast<const uint16_t *>(call.host_init);
        for (size_t k = 0; k < (size_t)call.R * p->n; ++k)
            if (l[k] >= (uint16_t)p->K) return fail(MI_EINVAL, "initial label %u >= K = %d", (unsigned)l[k], p->K);
    }
    // the kernel of this call, decided in one place (csrc/mi_sa_plan.h)
    RunFacts run;
    run.R = call.R; run.cus = p->cus; run.pair_weight_slot = a.wslot; run.node_weights = p->nw.d_nwq != nullptr; run.min_cluster_size = a.min_size;
    AnnealPlan plan;
    std::string plan_err;
    if (const int rc_p = plan_anneal(m.facts, run, p->opt.plan, &plan, &plan_err)) return fail(rc_p, "%s", plan_err.c_str());
    a.adj4 = m.packing(plan.packing); a.ring_off = plan.ring_off;
    p->last.adj_bytes = plan.adj_bytes;
    HIP_TRY(hipEventRecord(p->ev.e[0], p->stream));
    MI_TRY(call.merges ? anneal_potts_with_merges(p, call, a, plan) : launch_structured(plan, a, p->stream));
    HIP_TRY(hipEventRecord(p->ev.e[1], p->stream));
    return MI_OK;
}

}  // namespace

extern "C" {

int mi_sa_anneal_ex(mi_sa_problem *p, int R, uint32_t replica_offset, int num_sweeps,
                    const double *betas, uint64_t seed, const void *init, int resync_interval,
                    uint32_t sweep_offset, uint32_t flags)
{
    return on_problem(p, NO_ARGS, ON_DEVICE, [&]() -> int {
        AnnealCall call;
        MI_TRY(stage_anneal(p, R, replica_offset, num_sweeps, betas, seed, init, resync_interval, sweep_offset, flags, &call));
        MI_TRY(p->kind != MI_KIND_DENSE ? anneal_structured(p, call) : (p->xl.chunks > 0 ? anneal_dense_xl(p, call) : anneal_dense(p, call)));
        // what ran (a cooling run still in its worker reports its kernels when it is joined: settle)
        p->last.R = R; p->last.offset = replica_offset; p->last.has_run = true;
        p->last.kernel = g_kernel;
        return MI_OK;
    });
}

int mi_sa_anneal(mi_sa_problem *p, int R, uint32_t replica_offset, int num_sweeps,
                 const double *betas, uint64_t seed, const void *init, int resync_interval)
{
    return mi_sa_anneal_ex(p, R, replica_offset, num_sweeps, betas, seed, init, resync_interval, 0u, 0u);
}

int mi_sa_tempering_begin(mi_sa_problem *p, const double *ladder_betas, int T, int chains,
                          uint32_t first_replica, int R_local)
{
    return on_problem(p, ladder_betas != nullptr, STREAM_IDLE, [&]() -> int {
        if (p->nw.ngroups > 1) return fail(MI_EUNSUPPORTED, "tempering with resolution groups is not supported");
        if (p->merge.interval > 0) return fail(MI_EUNSUPPORTED, "tempering with merge moves is not supported");
        if (T < 2 || T > 1024) return fail(MI_EINVAL, "a tempering ladder has 2 .. 1024 temperatures (got %d)", T);
        if (chains < 1) return fail(MI_EINVAL, "chains must be >= 1");
        const long long total = (long long)T * chains;
        if (R_local < 1 || (long long)first_replica + R_local > total)
            return fail(MI_EINVAL, "local replicas [%u, %u + %d) do not lie inside the %lld replicas of the run", first_replica, first_replica, R_local, total);
        for (int k = 0; k < T; ++k)
            if (!(ladder_betas[k] > 0.0) || !std::isfinite(ladder_betas[k]))
                return fail(MI_EINVAL, "ladder beta %d = %g is not a positive finite number", k, ladder_betas[k]);
        MI_TRY(ensure_run_buffers(p, R_local, R_local, false));
        mi_sa_problem::Tempering &t = p->pt;
        t.T = 0;                                 // no tempering is set up until all of it is: a failure clears the rest
        const int rc = guarded([&]() -> int {
            std::vector<int> rung((size_t)total);
            for (long long g = 0; g < total; ++g) rung[(size_t)g] = (int)(g % T);
            std::vector<float> lt((size_t)T), local((size_t)R_local);
            for (int k = 0; k < T; ++k) lt[(size_t)k] = (float)(1.0 / ladder_betas[k]);
            for (int r = 0; r < R_local; ++r) local[(size_t)r] = lt[(size_t)(((long long)first_replica + r) % T)];
            HIP_TRY(t.d_rung.upload(rung));
            HIP_TRY(t.d_betas.upload(ladder_betas, (size_t)T));
            HIP_TRY(t.d_energy.resize((size_t)total));
            HIP_TRY(t.d_ladder.upload(lt));
            HIP_TRY(t.d_temps.upload(local));
            HIP_TRY(t.d_stats.resize(2));
            HIP_TRY(hipMemset(t.d_stats, 0, 2 * sizeof(unsigned long long)));
            return MI_OK;
        });
        if (rc) { t.clear(); return rc; }
        t.T = T; t.chains = chains; t.lo = (int)first_replica; t.R_local = R_local;
        return MI_OK;
    });
}

static int tempering_exchange_impl(mi_sa_problem *p, uint32_t round, uint64_t seed, const double *all_energies, bool on_device)
{
    return on_problem(p, NO_ARGS, ON_DEVICE, [&]() -> int {
        const mi_sa_problem::Tempering &t = p->pt;
        if (t.T == 0) return fail(MI_ESTATE, "mi_sa_tempering_begin has not been called on this problem");
        if (!p->last.has_run || p->last.R != t.R_local) return fail(MI_ESTATE, "no tempering round has run on this problem");
        const long long total = (long long)t.T * t.chains;
        if (!all_energies && t.R_local != total)
            return fail(MI_EINVAL, "this GPU holds %d of the %lld replicas: the exchange needs all energies", t.R_local, total);
        const double *en = p->run.d_energy;          // one GPU owns every replica: the energies never leave HBM
        if (all_energies && on_device) {
            en = all_energies;                       // the all-gather's output buffer, already in HBM
        } else if (all_energies) {
            HIP_TRY(hipMemcpyAsync(t.d_energy, all_energies, (size_t)total * sizeof(double), hipMemcpyHostToDevice, p->stream));
            en = t.d_energy;
        }
        hipLaunchKernelGGL(k_pt_exchange, dim3(t.chains), dim3(256), (size_t)t.T * sizeof(int), p->stream.st, en,
                           t.d_rung.p, t.d_betas.p, t.d_ladder.p, t.d_temps.p, t.T, t.lo, t.lo + t.R_local,
                           round, (uint32_t)seed, (uint32_t)(seed >> 32), t.d_stats.p);
        HIP_TRY(hipGetLastError());
        if (all_energies) HIP_TRY(hipStreamSynchronize(p->stream));      // the caller's buffer may go away
        return MI_OK;
    });
}

int mi_sa_tempering_exchange(mi_sa_problem *p, uint32_t round, uint64_t seed, const double *all_energies)
{
    return tempering_exchange_impl(p, round, seed, all_energies, false);
}

int mi_sa_tempering_exchange_dev(mi_sa_problem *p, uint32_t round, uint64_t seed, const double *d_all_energies)
{
    if (!d_all_energies) return guarded([]() -> int { return fail(MI_EINVAL, "d_all_energies is NULL"); });
    return tempering_exchange_impl(p, round, seed, d_all_energies, true);
}

int mi_sa_device_results(mi_sa_problem *p, void **out_d_states, double **out_d_energy, int *out_R)
{
    return on_problem(p, NO_ARGS, NEED_RUN | STREAM_IDLE, [&]() -> int {
        if (out_d_states) *out_d_states = p->run.d_states;
        if (out_d_energy) *out_d_energy = p->run.d_energy;
        if (out_R) *out_R = p->last.R;
        return MI_OK;
    });
}

int mi_sa_tempering_state(mi_sa_problem *p, int32_t *out_rung, uint64_t *out_proposed, uint64_t *out_accepted)
{
    return on_problem(p, NO_ARGS, STREAM_IDLE, [&]() -> int {
        const mi_sa_problem::Tempering &t = p->pt;
        if (t.T == 0) return fail(MI_ESTATE, "mi_sa_tempering_begin has not been called on this problem");
        if (out_rung)
            HIP_TRY(hipMemcpy(out_rung, t.d_rung, (size_t)t.T * t.chains * sizeof(int), hipMemcpyDeviceToHost));
        unsigned long long st[2];
        HIP_TRY(hipMemcpy(st, t.d_stats, sizeof st, hipMemcpyDeviceToHost));
        if (out_proposed) *out_proposed = st[0];
        if (out_accepted) *out_accepted = st[1];
        return MI_OK;
    });
}

int mi_sa_sync(mi_sa_problem *p)
{
    return on_problem(p, NO_ARGS, STREAM_IDLE, []() -> int { return MI_OK; });
}

int mi_sa_last_kernel_ms(mi_sa_problem *p, float *out_ms)
{
    return on_problem(p, out_ms != nullptr, NEED_RUN | ON_DEVICE, [&]() -> int {
        HIP_TRY(hipEventSynchronize(p->ev.e[1]));
        HIP_TRY(hipEventElapsedTime(out_ms, p->ev.e[0], p->ev.e[1]));
        return MI_OK;
    });
}

int mi_sa_last_launch_count(mi_sa_problem *p, int *out_launches)
{
    return on_problem(p, out_launches != nullptr, NEED_RUN, [&]() -> int {
        *out_launches = p->last.launches;
        return MI_OK;
    });
}

int mi_sa_last_adjacency_bytes_per_slot(mi_sa_problem *p, int *out_bytes)
{
    return on_problem(p, out_bytes != nullptr, NEED_RUN, [&]() -> int {
        *out_bytes = p->last.adj_bytes;
        return MI_OK;
    });
}

int mi_sa_last_kernel_name(mi_sa_problem *p, char *out, int len)
{
    return on_problem(p, out && len >= 1, NEED_RUN, [&]() -> int {
        snprintf(out, (size_t)len, "%s", p->last.kernel.c_str());
        return MI_OK;
    });
}

int mi_sa_fetch(mi_sa_problem *p, void *out_states, double *out_energy, uint64_t *out_stats)
{
    return on_problem(p, NO_ARGS, NEED_RUN | STREAM_IDLE, [&]() -> int {
        if (out_states)
            HIP_TRY(hipMemcpy(out_states, p->run.d_states, (size_t)p->last.R * p->n * p->state_elem, hipMemcpyDeviceToHost));
        if (out_energy)
            HIP_TRY(hipMemcpy(out_energy, p->run.d_energy, (size_t)p->last.R * sizeof(double), hipMemcpyDeviceToHost));
        if (out_stats) {
            unsigned long long st[4];
            HIP_TRY(hipMemcpy(st, p->run.d_stats, sizeof st, hipMemcpyDeviceToHost));
            out_stats[0] = st[0]; out_stats[1] = st[1]; out_stats[2] = st[2];
        }
        return MI_OK;
    });
}

int mi_sa_problem_label_agreement(mi_sa_problem *p, int groups, double *out_ari, double *out_nmi, int64_t *out_pair_sum,
                                  float *out_kernel_ms)
{
    return on_problem(p, NO_ARGS, NEED_RUN | ON_DEVICE, [&]() -> int {
        if (p->kind != MI_KIND_POTTS_CSR) return fail(MI_ESTATE, "label agreement needs a Potts problem");
        const int G = groups > 0 ? groups : p->nw.ngroups;
        if (p->last.R % G != 0) return fail(MI_EINVAL, "R = %d is not a multiple of groups = %d", p->last.R, G);
        int n_real = 0;
        for (int i = 0; i < p->n; ++i) n_real += (p->slot.h_meta[(size_t)i] >> 31) ? 0 : 1;
        if (n_real < 1) return fail(MI_EINVAL, "every variable of the problem is a hole");
        const void *labels = p->run.d_states;
        AgreeArgs a;
        a.A = static_cast<const uint16_t *>(labels); a.lda = (size_t)p->n;
        a.Ra = p->last.R; a.cols = p->n; a.Ka = a.Kb = p->K; a.groups = G;
        a.meta = p->slot.d_meta; a.n_real = n_real;
        return mi_label_agreement_dev(a, p->stream, out_ari, out_nmi, out_pair_sum, nullptr, out_kernel_ms);
    });
}

int mi_sa_problem_coassociation(mi_sa_problem *p, int groups, const uint16_t *ref, int Kref, const int32_t *eu,
                                const int32_t *ev, int64_t m, int64_t *out_hist, int64_t *out_rowsum, int32_t *out_edge,
                                int32_t *out_counts, float *out_kernel_ms)
{
    return on_problem(p, NO_ARGS, NEED_RUN | ON_DEVICE, [&]() -> int {
        if (p->kind != MI_KIND_POTTS_CSR) return fail(MI_ESTATE, "co-association needs a Potts problem");
        const int G = groups > 0 ? groups : p->nw.ngroups;
        MI_TRY(mi_coassociation_check(p->last.R, p->n, p->K, G, ref, Kref, eu, ev, m, out_rowsum, out_edge));
        const void *labels = p->run.d_states;
        CoassocArgs a;
        a.L = static_cast<const uint16_t *>(labels); a.ld = (size_t)p->n;
        a.R = p->last.R; a.cols = p->n; a.K = p->K; a.groups = G; a.meta = p->slot.d_meta;
        a.ref = ref; a.Kref = ref ? Kref : 1; a.eu = eu; a.ev = ev; a.m = out_edge ? m : 0;
        return mi_coassociation_dev(a, p->stream, out_hist, out_rowsum, out_edge, out_counts, out_kernel_ms);
    });
}

int mi_sa_problem_components(mi_sa_problem *p, int32_t *out_labels, int32_t *out_count, float *out_kernel_ms)
{
    return on_problem(p, NO_ARGS, NEED_RUN | ON_DEVICE, [&]() -> int {
        if (!out_labels || !out_count) return fail(MI_EINVAL, "NULL argument");
        if (p->kind != MI_KIND_POTTS_CSR) return fail(MI_ESTATE, "components need a Potts problem");
        const void *labels = p->run.d_states;
        ComponentsArgs a;
        a.rows = p->slot.d_rows; a.meta = p->slot.d_meta; a.D = p->slot.D; a.n = p->n;
        a.L = static_cast<const uint16_t *>(labels); a.ldl = (size_t)p->n;
        return mi_components_dev(a, p->last.R, false, p->stream, out_labels, out_count, out_kernel_ms);
    });
}

int mi_sa_best(mi_sa_problem *p, int *out_index, double *out_energy, uint64_t *out_key, void *out_state)
{
    return on_problem(p, NO_ARGS, NEED_RUN | ON_DEVICE, [&]() -> int {
        if (p->nw.ngroups > 1) return fail(MI_EUNSUPPORTED, "best of a run with resolution groups: one minimum across different objectives");
        const mi_sa_problem::Run &b = p->run;
        unsigned long long init_key = ~0ull, key = 0;
        HIP_TRY(hipMemcpyAsync(b.d_stats + 3, &init_key, sizeof init_key, hipMemcpyHostToDevice, p->stream));
        hipLaunchKernelGGL(k_best, dim3(1), dim3(1024), 0, p->stream.st, b.d_energy.p, p->last.R, p->last.offset, b.d_stats + 3);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(&key, b.d_stats + 3, sizeof key, hipMemcpyDeviceToHost, p->stream));
        HIP_TRY(hipStreamSynchronize(p->stream));
        const int idx = (int)((uint32_t)(key & 0xffffffffull) - p->last.offset);
        if (idx < 0 || idx >= p->last.R) return fail(MI_EHIP, "best-of reduction returned an invalid index %d", idx);
        if (out_index) *out_index = idx;
        if (out_key) *out_key = key;
        const size_t replica_bytes = (size_t)p->n * p->state_elem;
        if (out_energy) HIP_TRY(hipMemcpy(out_energy, b.d_energy + idx, sizeof(double), hipMemcpyDeviceToHost));
        if (out_state) HIP_TRY(hipMemcpy(out_state, b.d_states + (size_t)idx * replica_bytes, replica_bytes, hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

// ---- several GPUs from ONE process (callers without a process-per-GPU launcher) -------------------------------
// Replicas are independent chains: problem d (the same model created on device d) runs the contiguous shard d of the
// global replica ids; the anneals are asynchronous on each device's own stream, so the devices run concurrently; the
// best replica is the minimum of the per-device packed keys -- the same reduction distributed.global_best does with one
// RCCL all-reduce when there is one process per GPU.
static void shard_of(int R_total, int d, int ndev, int *lo, int *hi)
{
    const int base = R_total / ndev, rem = R_total % ndev;
    *lo = d * base + (d < rem ? d : rem);
    *hi = *lo + base + (d < rem ? 1 : 0);
}

static int multi_check(mi_sa_problem *const *problems, int ndev)
{
    if (!problems || ndev < 1) return fail(MI_EINVAL, "need ndev >= 1 problem handles");
    for (int d = 0; d < ndev; ++d) {
        if (!problems[d]) return fail(MI_EINVAL, "problem %d is NULL", d);
        if (problems[d]->nw.ngroups > 1) return fail(MI_EUNSUPPORTED, "problem %d has resolution groups: not sharded over GPUs", d);
        if (problems[d]->kind != problems[0]->kind || problems[d]->n != problems[0]->n || problems[d]->K != problems[0]->K)
            return fail(MI_EINVAL, "problem %d is not the model of problem 0 (kind / size differ)", d);
    }
    return MI_OK;
}

int mi_multi_gpu_anneal(mi_sa_problem *const *problems, int ndev, int R_total, uint32_t replica_offset,
                        int num_sweeps, const double *betas, uint64_t seed, int resync_interval)
{
    return guarded([&]() -> int {
        MI_TRY(multi_check(problems, ndev));
        if (R_total < ndev) return fail(MI_EINVAL, "R_total = %d replicas cannot be sharded over %d devices", R_total, ndev);
        for (int d = 0; d < ndev; ++d) {
            int lo, hi;
            shard_of(R_total, d, ndev, &lo, &hi);
            MI_TRY(mi_sa_anneal_ex(problems[d], hi - lo, replica_offset + (uint32_t)lo, num_sweeps, betas, seed, nullptr,
                                   resync_interval, 0u, 0u));
        }
        return MI_OK;
    });
}

int mi_multi_gpu_best(mi_sa_problem *const *problems, int ndev, int *out_owner, uint32_t *out_global_id,
                      double *out_energy, void *out_state)
{
    return guarded([&]() -> int {
        MI_TRY(multi_check(problems, ndev));
        // one process sees every device's exact fp64 minimum: lowest energy, ties to the lowest global id (the devices
        // hold ascending id ranges) -- the record a sorted SampleSet of all replicas puts first
        int owner = -1, best_idx = 0;
        uint64_t best_key = ~0ull;
        double best_e = 0.0;
        for (int d = 0; d < ndev; ++d) {
            int idx = 0;
            uint64_t key = 0;
            double e = 0.0;
            MI_TRY(mi_sa_best(problems[d], &idx, &e, &key, nullptr));
            if (owner < 0 || e < best_e) { owner = d; best_key = key; best_idx = idx; best_e = e; }
        }
        mi_sa_problem *p = problems[owner];
        HIP_TRY(hipSetDevice(p->device));
        if (out_owner) *out_owner = owner;
        if (out_global_id) *out_global_id = (uint32_t)(best_key & 0xffffffffull);
        const size_t replica_bytes = (size_t)p->n * p->state_elem;
        if (out_energy) HIP_TRY(hipMemcpy(out_energy, p->run.d_energy + best_idx, sizeof(double), hipMemcpyDeviceToHost));
        if (out_state)
            HIP_TRY(hipMemcpy(out_state, p->run.d_states + (size_t)best_idx * replica_bytes, replica_bytes, hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_multi_gpu_fetch(mi_sa_problem *const *problems, int ndev, void *out_states, double *out_energy, uint64_t *out_stats)
{
    return guarded([&]() -> int {
        MI_TRY(multi_check(problems, ndev));
        size_t done = 0;
        uint64_t tot[3] = {0, 0, 0};
        for (int d = 0; d < ndev; ++d) {
            mi_sa_problem *p = problems[d];
            if (!p->last.has_run) return fail(MI_ESTATE, "no anneal has been run on problem %d", d);
            uint64_t st[3] = {0, 0, 0};
            MI_TRY(mi_sa_fetch(p, out_states ? (char *)out_states + done * p->n * p->state_elem : nullptr,
                               out_energy ? out_energy + done : nullptr, st));
            for (int k = 0; k < 3; ++k) tot[k] += st[k];
            done += (size_t)p->last.R;
        }
        if (out_stats) { out_stats[0] = tot[0]; out_stats[1] = tot[1]; out_stats[2] = tot[2]; }
        return MI_OK;
    });
}

int mi_sa_qubo_dense_f32(const float *Qs, int n, double offset, int R, int num_sweeps,
                         const double *betas, uint64_t seed, const uint8_t *init,
                         uint8_t *out_states, double *out_energy, uint64_t *out_stats, int device)
{
    mi_sa_problem *p = nullptr;
    int rc = mi_sa_problem_create_dense_f32(Qs, n, offset, device, &p);
    if (rc) return rc;
    rc = mi_sa_anneal(p, R, 0, num_sweeps, betas, seed, init, 0);
    if (!rc) rc = mi_sa_fetch(p, out_states, out_energy, out_stats);
    if (!rc && out_stats) out_stats[0] = (uint64_t)R * (uint64_t)num_sweeps * (uint64_t)n;
    mi_sa_problem_destroy(p);
    return rc;
}

// K4's states are bytes 0 / 1.  The VALU form takes any non-zero byte as set, the MFMA form multiplies by the byte's value
// and masks with its bit 0: another byte (255 from a -1 spin cast to uint8) would give energies that depend on the path,
// so it is refused.  One pass that ORs the high seven bits of every byte, and a search only when one is set.
static int check_state_bytes(const uint8_t *X, int n, int R)
{
    const size_t total = (size_t)R * n;
    unsigned int high = 0u;
    for (size_t e = 0; e < total; ++e) high |= X[e];
    if (!(high & 0xfeu)) return MI_OK;
    size_t e = 0;
    while (X[e] <= 1) ++e;
    return fail(MI_EINVAL, "states must be bytes 0 or 1: cell %lld of state %lld is %d", (long long)(e % n), (long long)(e / n), (int)X[e]);
}

int mi_energy_dense_f32_ex(const float *Qs, int n, const uint8_t *X, int R, double offset,
                           double *out_energy, int device, int path, float *out_kernel_ms)
{
    if (!Qs || !X || !out_energy) return fail(MI_EINVAL, "NULL argument");
    if (n < 1 || R < 1) return fail(MI_EINVAL, "n and R must be >= 1");
    if (path < 0 || path > 2) return fail(MI_EINVAL, "path must be 0 (auto), 1 (VALU) or 2 (MFMA)");
    MI_TRY(check_state_bytes(X, n, R));
    if (path != 1 && (path == 2 || R >= 32)) {
        // the MFMA kernel multiplies only the blocks on and above the diagonal of a SYMMETRIC Qs: a matrix that is not
        // (e.g. an upper-triangular QUBO) goes to the exact path when the choice is the library's, and is refused when
        // the caller asked for the MFMA path by name
        bool symmetric = true;
        for (int i = 0; i < n && symmetric; ++i)
            for (int j = i + 1; j < n; ++j)
                if (Qs[(size_t)i * n + j] != Qs[(size_t)j * n + i]) { symmetric = false; break; }
        if (!symmetric) {
            if (path == 2) return fail(MI_EINVAL, "the MFMA energy path (path = 2) needs a symmetric Qs; use (Q + Q^T) / 2 or path 0 / 1");
            path = 1;
        }
    }
    if (path == 0) path = (R >= 32) ? 2 : 1;      // MFMA only when the batch is a real dense contraction
    MI_TRY(pick_device(device));
    return guarded([&]() -> int {
        DevBufs bufs;
        float *dQ = nullptr; uint8_t *dX = nullptr, *dXt = nullptr; double *dE = nullptr;
        // the MFMA kernel reads whole 128 x 128 blocks: rows padded to n_pad floats, n_pad rows, padding zero
        const size_t ldq = path == 2 ? ((size_t)n + 127) / 128 * 128 : (size_t)n;
        const size_t rows = path == 2 ? ldq : (size_t)n;
        HIP_TRY(bufs.alloc(&dQ, rows * ldq));
        HIP_TRY(bufs.upload(&dX, X, (size_t)R * n));
        HIP_TRY(bufs.alloc(&dE, (size_t)R));
        if (path == 2) {
            HIP_TRY(bufs.alloc(&dXt, mi_energy_dense_scratch_bytes(n, R)));
            HIP_TRY(hipMemset(dQ, 0, rows * ldq * sizeof(float)));
        }
        HIP_TRY(hipMemcpy2D(dQ, ldq * sizeof(float), Qs, (size_t)n * sizeof(float), (size_t)n * sizeof(float), (size_t)n,
                            hipMemcpyHostToDevice));
        Timer tm;
        MI_TRY(tm.start(0));
        MI_TRY(mi_launch_energy_dense(dQ, n, (int)ldq, dX, R, offset, dE, dXt, path, 0));
        MI_TRY(tm.stop(0, out_kernel_ms));
        HIP_TRY(hipMemcpy(out_energy, dE, (size_t)R * sizeof(double), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_energy_dense_f64(const double *Qs, int n, const uint8_t *X, int R, double offset,
                        double *out_energy, int device)
{
    if (!Qs || !X || !out_energy) return fail(MI_EINVAL, "NULL argument");
    if (n < 1 || R < 1) return fail(MI_EINVAL, "n and R must be >= 1");
    MI_TRY(check_state_bytes(X, n, R));
    MI_TRY(pick_device(device));
    return guarded([&]() -> int {
        DevBufs bufs;
        double *dQ = nullptr, *dE = nullptr; uint8_t *dX = nullptr;
        HIP_TRY(bufs.upload(&dQ, Qs, (size_t)n * n));
        HIP_TRY(bufs.upload(&dX, X, (size_t)R * n));
        HIP_TRY(bufs.alloc(&dE, (size_t)R));
        MI_TRY(mi_launch_energy_dense_f64(dQ, n, dX, R, offset, dE, 0));
        HIP_TRY(hipMemcpy(out_energy, dE, (size_t)R * sizeof(double), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

int mi_energy_dense_f32(const float *Qs, int n, const uint8_t *X, int R, double offset,
                        double *out_energy, int device)
{
    return mi_energy_dense_f32_ex(Qs, n, X, R, offset, out_energy, device, 0, nullptr);
}

}  // extern "C"
