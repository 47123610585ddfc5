// Stand-alone host program over the HIP-free headers of the engine (csrc/mi_sa_plan.h, csrc/mi_dense_plan.h,
// csrc/mi_sa_pack.h): the model facts, both planners and every packer at the edge shapes -- n = 1, 63, 64, 65, an empty
// graph, max degree 0, 13, 15, 16, 17, 64, 65, 4096, and 4097, which must be refused -- with the sizes of what they return
// checked; the dense planner at every register width, ring unit and occupancy (check_dense).  Built with
// -fsanitize=address,undefined by tests/test_plan_pack_host.py; prints "ok" and returns 0.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_sa_pack.h"
#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_sa_plan.h"
#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_dense_plan.h"

using namespace mi_sa_plan;

#define CHECK(cond)                                                                     \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            fprintf(stderr, "%s:%d: check failed: %s\n", __FILE__, __LINE__, #cond);    \
            exit(1);                                                                    \
        }                                                                               \
    } while (0)

struct Csr {
    int n;
    std::vector<int32_t> rowptr, col;
    std::vector<float> val;
};

// `hubs` nodes of degree `degree`, each joined to the `degree` nodes that follow at distance >= gap (symmetric);
// gap = 1: edges inside slots; gap = 64: none
static Csr hub_graph(int n, int degree, int gap)
{
    std::vector<std::vector<int>> adj((size_t)n);
    if (degree > 0) {
        CHECK(n >= gap + degree);
        for (int k = 0; k < degree; ++k) {
            adj[0].push_back(gap + k);
            adj[(size_t)(gap + k)].push_back(0);
        }
    }
    Csr g;
    g.n = n;
    g.rowptr.push_back(0);
    for (int i = 0; i < n; ++i) {
        for (int j : adj[(size_t)i]) { g.col.push_back(j); g.val.push_back(1.0f + (float)j); }
        g.rowptr.push_back((int32_t)g.col.size());
    }
    return g;
}

static int plans_checked = 0;

// (pack_all: every packer at every state width; else one image -- the widest rows take 70 MB each)
static void check_model(int kind, const Csr &g, int K, const char *forced_state, bool pack_all = true)
{
    std::string err;
    SlotModelFacts f;
    int degree = 0;
    for (int i = 0; i < g.n; ++i) degree = std::max(degree, g.rowptr[(size_t)i + 1] - g.rowptr[(size_t)i]);
    const int rc = slot_model_facts(kind, g.rowptr.data(), g.col.data(), g.n, K, forced_state, &f, &err);
    if (degree > 4096) {
        CHECK(rc == MI_EUNSUPPORTED && err.find("max degree 4097") != std::string::npos);
        return;
    }
    CHECK(rc == MI_OK);
    CHECK(f.max_degree == degree && f.slots == (g.n + 63) / 64 && f.D >= degree && f.D % 16 == 0 && f.D >= 16);
    CHECK(f.D == 16 || f.D == 32 || f.D == 64 || (f.D > 64 && f.D - degree < 16));
    CHECK(!f.has_pair16 || f.has_pair_packing);
    CHECK(f.trim_rw == 0 || (f.has_pair_packing && f.trim_rw == degree && degree >= 13 && degree <= 15));
    CHECK(!(f.has_pair_packing && f.has_fast_packing));

    std::vector<uint32_t> hc;
    std::vector<float> hv;
    build_slot_ell(g.rowptr.data(), g.col.data(), g.val.data(), g.n, f.slots, f.D, hc, hv);
    CHECK(hc.size() == (size_t)f.slots * f.D * 64 && hv.size() == hc.size());
    const size_t image = (size_t)f.slots * (f.D / 4) * 2 * 256;
    for (int sb : {2, 1, 0}) {
        if (!pack_all && sb != f.state_bytes) continue;
        CHECK(pack_groups_of_four(hc, hv, f.slots, f.D, [&](uint32_t c, int, int) { return k2_state_word(c, sb); }).size() == image);
    }
    if (f.has_pair_packing || f.has_fast_packing)
        CHECK(pack_groups_of_four(hc, hv, f.slots, f.D, [](uint32_t c, int, int) { return 4u * c; }).size() == image);
    if (f.has_pair16) CHECK(pack_pair_adjacency16(hc, hv, f.slots, f.D).size() == (size_t)f.slots * (f.D / 8 + f.D / 4) * 256);
    if (f.trim_rw) {
        const size_t last = f.trim_rw == 15 ? 448 : (size_t)(f.trim_rw - 12) * 128;
        CHECK(pack_pair_adjacency(hc, hv, f.slots, f.D, f.trim_rw).size() == (size_t)f.slots * (3 * 512 + last));
    }

    for (int R : {1, 2, 1024, 1025, 3586, 4098, 7374})
        for (int v = 0; v < 3; ++v)
            for (const char *key : {"k2_pair", "k2_split", "k2_wide", "k2_tw", "k2_trim", "k2_nbr16", "k3_fast"})
                for (int weighted = 0; weighted < 2; ++weighted) {
                    PlanOptions o;
                    CHECK(plan_option_set(o, key, v));
                    RunFacts run;
                    run.R = R; run.cus = 256;
                    run.pair_weight_slot = weighted && kind == MI_KIND_CSR_RANK1 ? f.slots - 1 : -1;
                    run.node_weights = weighted && kind == MI_KIND_POTTS_CSR;
                    run.min_cluster_size = weighted ? 0 : v;
                    AnnealPlan p;
                    if (plan_anneal(f, run, o, &p, &err) != MI_OK) { CHECK(!err.empty()); continue; }
                    char name[128] = "";
                    plan_kernel_name(p, name, sizeof name);
                    CHECK(name[0] == 'k' && p.lds_bytes <= kLdsBytes && p.grid >= 1 && p.block >= 64 && p.block % 64 == 0);
                    CHECK((p.adj_bytes != 0) == (p.family == PLAN_K2P));
                    ++plans_checked;
                }
}

// The dense planner at every width NT, ring unit and a synthetic occupancy: K1's launches cover the replicas exactly, within
// kMaxChunks, and are paced only where they are co-resident; the steps of a plan tile [0, num_sweeps); the ring arithmetic
// gives the refusals tests/golden/dense_plan_table.json recorded (4 rows from NT = 56, K1m above NT = 44).
static void check_dense()
{
    for (int NT = 4; NT <= 64; NT += 4) {
        CHECK(dense_ring_units(NT, 2) >= 3 && (dense_ring_units(NT, 4) >= 3) == (NT <= 52) && dense_ring_units(NT, 3) == 0);
        for (int GR : {2, 4}) CHECK(dense_ring_units(NT, GR) * GR * NT * 256 <= kDenseRingBytes && (dense_ring_units(NT, GR) - 2) * GR < 64);
    }
    CHECK(dense_ring_units(4, 4) == 17 && dense_ring_units(4, 2) == 32 && dense_ring_units(48, 4) == 3 && dense_ring_units(64, 2) == 4);
    for (int NT = 4; NT <= 64; NT += 4)
        for (int n : {64 * NT - 255, 64 * NT})
            for (int GR : {0, 2, 4})
                for (int waves : {4, 8, 1000})
                    for (int variant = 0; variant <= 4; ++variant)
                        for (int chunk : {0, 1, 2, 32})
                            for (int sweeps : {0, 1, 2, 3, 5, 32, 33, 4086, 4087})
                                for (int R : {1, 4, 5, 19, 31, 32, 127, 128, 1000, 1024, 1025, 64 * 1000, 64 * 1000 + 1})
                                    for (int pace : {0, 1}) {
                                        DensePlanOptions o;
                                        CHECK(dense_plan_option_set(o, "variant", variant) && dense_plan_option_set(o, "unit_rows", GR));
                                        CHECK(dense_plan_option_set(o, "chunk_sweeps", chunk) && dense_plan_option_set(o, "pace", 7 * pace));
                                        DenseRun run;
                                        run.n = n; run.R = R; run.num_sweeps = sweeps; run.cus = 256; run.resident_waves = waves;
                                        DensePlan p;
                                        std::string err;
                                        CHECK(dense_width(n) == NT);
                                        const int rc = plan_dense(run, o, &p, &err);
                                        ++plans_checked;
                                        if (rc != MI_OK) {
                                            // the refusals: K1m above NT = 44, a ring unit that does not fit, too many launches to schedule
                                            CHECK(!err.empty() && variant != 1);
                                            const bool k1m = NT > kMaxMfmaNT && (variant == 3 || variant == 4);
                                            const bool ring = GR == 4 && NT >= 56 && variant != 3;
                                            const bool sched = (variant == 4 || variant == 0) && chunk == 1 && sweeps == 4087 && R >= 32;
                                            CHECK(k1m || ring || sched);
                                            CHECK(rc == (err.find("too many chunks") != std::string::npos ? MI_EINVAL : MI_EUNSUPPORTED));
                                            continue;
                                        }
                                        char name[128];
                                        dense_plan_kernel_name(p, name, sizeof name);
                                        CHECK(name[0] == 'k' && p.NT == NT && p.num_sweeps == sweeps);
                                        CHECK((p.form == DENSE_K1) == dense_plan_is_k1(run, o));
                                        if (p.form == DENSE_K1) {
                                            CHECK(!p.cut && p.steps == 1 && p.field_floats == 0 && p.unit_rows == 0);
                                            CHECK(p.launches >= 1 && p.launches <= kMaxChunks && p.replicas_per_launch >= 1);
                                            int covered = 0, count = 0;
                                            for (int lo = 0; lo < R; lo += p.replicas_per_launch, ++count) {
                                                const int cnt = std::min(R - lo, p.replicas_per_launch);
                                                CHECK(cnt >= 1 && (!dense_k1_paced(p, cnt) || (cnt <= waves && pace && sweeps > 1)));
                                                covered += cnt;
                                            }
                                            CHECK(covered == R && count == p.launches);
                                            CHECK(p.replicas_per_launch == waves || p.launches == kMaxChunks || (R + waves - 1) / waves > kMaxChunks);
                                        } else {
                                            CHECK(p.launches == p.steps && p.cut == (p.steps > 1) && (p.field_floats != 0) == p.cut);
                                            CHECK(!p.cut || (p.field_floats == (size_t)R * NT * 64 && chunk > 0 && sweeps > chunk && R >= 32));
                                            CHECK((p.form == DENSE_K1M) == (p.unit_rows == 0) && (p.unit_rows == 0 || dense_ring_units(NT, p.unit_rows) >= 3));
                                            CHECK(p.form != DENSE_SCHEDULED || (p.cut && NT <= kMaxMfmaNT && p.steps + 2 <= kCtrlWords - kCtrlModes));
                                            CHECK(!p.wg_pace || (pace && (R + kWgWaves - 1) / kWgWaves <= 256));
                                        }
                                        // the steps tile [0, num_sweeps) without gap or overlap
                                        int at = 0;
                                        for (int i = 0; i < p.steps; ++i) {
                                            const DenseStep s = dense_plan_step(p, i);
                                            CHECK(s.s0 == at && s.first == (i == 0) && s.last == (i == p.steps - 1) && (s.len >= 1 || sweeps == 0));
                                            CHECK(!p.cut || s.len <= chunk);
                                            at += s.len;
                                        }
                                        CHECK(at == sweeps);
                                    }
    DenseRun run;
    DensePlan p;
    std::string err;
    run.n = 0;
    CHECK(plan_dense(run, DensePlanOptions(), &p, &err) == MI_EINVAL);
    run.n = 4097;
    CHECK(plan_dense(run, DensePlanOptions(), &p, &err) == MI_EUNSUPPORTED);
    DensePlanOptions o;
    CHECK(!dense_plan_option_set(o, "unit_rows", 3) && !dense_plan_option_set(o, "unit_rows", -2) && !dense_plan_option_set(o, "variant", 5));
    CHECK(!dense_plan_option_set(o, "xl_chunk", 2) && !dense_plan_option_set(o, "chunk_sweeps", -1) && !dense_plan_option_set(o, "k2_pair", 1));
    CHECK(dense_plan_option_set(o, "pace", -3) && o.pace == 1 && dense_plan_option_set(o, "pace", 0) && o.pace == 0);
}

int main()
{
    check_dense();
    for (int n : {1, 63, 64, 65}) {
        for (int kind : {MI_KIND_CSR_RANK1, MI_KIND_POTTS_CSR}) check_model(kind, hub_graph(n, 0, 1), 4, nullptr);   // an empty graph
        check_model(MI_KIND_CSR_RANK1, hub_graph(n, n > 1 ? 1 : 0, 1), 2, "bit");
    }
    for (int degree : {0, 13, 15, 16, 17, 64, 65, 4096, 4097})
        for (int gap : {1, 64})
            for (int kind : {MI_KIND_CSR_RANK1, MI_KIND_POTTS_CSR})
                for (const char *state : {(const char *)nullptr, "byte"}) {
                    if (degree >= 4096 && (gap != 1 || state)) continue;      // (the widest rows once per kind)
                    check_model(kind, hub_graph(gap + degree + (degree & 1), degree, gap), kind == MI_KIND_POTTS_CSR ? 9 : 2, state,
                                degree < 4096);
                }
    // the checks mi_sa_problem_create_* make first
    std::string err;
    CHECK(slot_model_size_check(MI_KIND_CSR_RANK1, 0, 2, &err) == MI_EINVAL);
    CHECK(slot_model_size_check(MI_KIND_POTTS_CSR, 40001, 4, &err) == MI_EUNSUPPORTED);
    CHECK(slot_model_size_check(MI_KIND_POTTS_CSR, 64, 65, &err) == MI_EUNSUPPORTED);
    // bad inputs are refused, not read past
    Csr g = hub_graph(65, 3, 1);
    SlotModelFacts f;
    g.col[0] = 65;
    CHECK(slot_model_facts(MI_KIND_CSR_RANK1, g.rowptr.data(), g.col.data(), g.n, 2, nullptr, &f, &err) == MI_EINVAL);
    g.col[0] = 0;
    CHECK(slot_model_facts(MI_KIND_CSR_RANK1, g.rowptr.data(), g.col.data(), g.n, 2, nullptr, &f, &err) == MI_EINVAL);
    g = hub_graph(65, 3, 1);
    g.rowptr[2] = g.rowptr[1] - 1;
    CHECK(slot_model_facts(MI_KIND_CSR_RANK1, g.rowptr.data(), g.col.data(), g.n, 2, nullptr, &f, &err) == MI_EINVAL);
    PlanOptions o;
    CHECK(!plan_option_set(o, "k2_pair", 3) && !plan_option_set(o, "pace", 1) && plan_option_set(o, "k2_waves", 99));
    CHECK(plans_checked > 1000);
    printf("ok: %d plans\n", plans_checked);
    return 0;
}
