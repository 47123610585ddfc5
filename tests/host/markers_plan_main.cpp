// Stand-alone host program over csrc/mi_markers_plan.h, the HIP-free plan of the marker ranking pass: the stored counts of
// a transpose, the LDS capacity and slab stride at the cap's edges, a plan by stored counts that differs from the plan by
// true counts, the forced HBM form, the grid under the slab budget, and random counts against the plan's invariants.
// Built with -fsanitize=address,undefined by tests/test_markers_sparse_host.py; prints "ok" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_markers_plan.h"

using namespace mi_markers_plan;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);    \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

static const int kCap = 8192, kChunk = 16, kCus = 256;              // MI_MARKERS_LDS_MAX_NONZEROS, MI_MARKERS_LABELLING_CHUNK
static const size_t kBudget = (size_t)1 << 30;

static Plan plan_of(const std::vector<int32_t> &counts, int K = 9, int cap = kCap, int cus = kCus, size_t budget = kBudget)
{
    return plan(counts.data(), (int)counts.size(), K, cap, kChunk, cus, budget);
}

static bool pow2(size_t v) { return v && !(v & (v - 1)); }

// what the kernels rely on: every gene's planned entries fit the array its form uses, the slabs fit the budget
static void check_invariants(const std::vector<int32_t> &counts, int K, int cap, int cus, size_t budget)
{
    const Plan p = plan_of(counts, K, cap, cus, budget);
    CHECK(p.lds_cap == 0 || (pow2((size_t)p.lds_cap) && p.lds_cap >= 16));
    CHECK(p.slab_stride == 0 || pow2(p.slab_stride));
    for (int32_t c : counts) {
        const size_t padded = c > 0 ? (size_t)next_pow2(c) : 0;
        if (c <= p.lds_cap) CHECK(padded <= (size_t)p.lds_cap);     // the kernel's rule: planned <= lds_cap -> LDS
        else CHECK(padded <= p.slab_stride);
        if (c <= cap) CHECK(c <= p.lds_cap);                         // at or below the cap a gene is always served in LDS
    }
    CHECK(p.lds_cap <= (cap > 16 ? next_pow2(cap) : 16));
    CHECK(p.lds_bytes % 16 == 0 && p.lds_bytes >= (size_t)p.lds_cap * 12 + (size_t)kChunk * K * 12);
    CHECK(p.lds_bytes <= (size_t)160 * 1024);
    CHECK(p.threads == 256 || p.threads == 1024);
    CHECK(p.grid >= 1 && (p.grid <= counts.size() || counts.empty()));
    CHECK(p.grid <= (size_t)(cus > 0 ? cus : 1) * 8);
    if (p.slab_stride && p.grid > 1) CHECK(p.grid * p.slab_stride * 12 <= budget);
}

static uint32_t rng_state = 2463534242u;
static uint32_t rnd()
{
    rng_state ^= rng_state << 13;
    rng_state ^= rng_state >> 17;
    rng_state ^= rng_state << 5;
    return rng_state;
}

int main()
{
    CHECK(next_pow2(0) == 1 && next_pow2(1) == 1 && next_pow2(2) == 2 && next_pow2(3) == 4 && next_pow2(256) == 256 &&
          next_pow2(257) == 512 && next_pow2(1 << 20) == 1 << 20);
    {
        const std::vector<int64_t> colptr = {0, 0, 3, 3, 10, 10};   // genes with 0, 3, 0, 7, 0 stored entries
        std::vector<int32_t> counts(5, -1);
        stored_counts(colptr.data(), 5, counts.data());
        CHECK((counts == std::vector<int32_t>{0, 3, 0, 7, 0}));
        const std::vector<int64_t> far = {(int64_t)1 << 31, ((int64_t)1 << 31) + (1 << 20)};      // positions past 2^31
        stored_counts(far.data(), 1, counts.data());
        CHECK(counts[0] == 1 << 20);
    }
    {
        const Plan p = plan_of({0, 0, 0});                           // no entry anywhere: no array, the accumulators only
        CHECK(p.lds_cap == 0 && p.slab_stride == 0 && p.lds_bytes == (size_t)kChunk * 9 * 12 && p.threads == 256 && p.grid == 3);
    }
    {
        const Plan p = plan_of({1, 0, 5});                           // the LDS arrays are never shorter than 16 entries
        CHECK(p.lds_cap == 16 && p.slab_stride == 0);
    }
    {
        const Plan p = plan_of({255, 256});
        CHECK(p.lds_cap == 256);
        const Plan q = plan_of({255, 257});                          // 257 stored, whatever the true count: planned for 512
        CHECK(q.lds_cap == 512 && q.threads == 256);
    }
    {
        const Plan p = plan_of({kCap, kCap + 1, 10}, 64);            // the last LDS gene, the first HBM gene
        CHECK(p.lds_cap == kCap && p.slab_stride == (size_t)2 * kCap && p.threads == 1024);
        CHECK(p.lds_bytes == (size_t)12 * 8192 + 12 * 16 * 64);      // 110 592 bytes at the cap, K = 64 (include/mi_metrics.h)
        const Plan q = plan_of({kCap, 10}, 64);
        CHECK(q.lds_cap == kCap && q.slab_stride == 0);
    }
    {
        const Plan p = plan_of({300, 17, 0}, 9, 0);                  // forced HBM form: a gene without entries still needs nothing
        CHECK(p.lds_cap == 0 && p.slab_stride == 512 && p.grid == 3);
    }
    {
        std::vector<int32_t> counts(5000, 100);                      // the grid: 8 workgroups per compute unit, at most g ...
        CHECK(plan_of(counts).grid == 2048 && plan_of({100, 100}).grid == 2 && plan_of(counts, 9, kCap, 0).grid == 8);
        counts[7] = 1 << 20;                                         // ... and as many 12 MiB slabs as the budget holds
        const Plan p = plan_of(counts);
        CHECK(p.slab_stride == (size_t)1 << 20 && p.grid == kBudget / (((size_t)1 << 20) * 12) && p.grid == 85);
        CHECK(plan_of(counts, 9, kCap, kCus, 1000).grid == 1);       // a budget below one slab still gives one workgroup
    }
    for (int round = 0; round < 200; ++round) {
        const int g = 1 + (int)(rnd() % 300), K = 1 + (int)(rnd() % 64);
        const int top = 1 << (rnd() % 21);                           // largest count up to 2^20 (MI_MARKERS_MAX_CELLS)
        std::vector<int32_t> counts((size_t)g);
        for (int32_t &c : counts) c = (rnd() & 3u) ? (int32_t)(rnd() % (uint32_t)(top + 1)) : 0;
        check_invariants(counts, K, (rnd() & 1u) ? kCap : 0, (int)(rnd() % 300), (rnd() & 7u) ? kBudget : (size_t)1 << 24);
    }
    printf("ok\n");
    return 0;
}
