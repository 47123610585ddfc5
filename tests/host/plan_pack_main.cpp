// Stand-alone host program over the HIP-free headers of the engine (csrc/mi_sa_plan.h, csrc/mi_sa_pack.h): the model
// facts, both planners and every packer at the edge shapes -- n = 1, 63, 64, 65, an empty graph, max degree 0, 13, 15, 16,
// 17, 64, 65, 4096, and 4097, which must be refused -- with the sizes of what they return checked.  Built with
// -fsanitize=address,undefined by tests/test_plan_pack_host.py; prints "ok" and returns 0.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_sa_pack.h"
#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_sa_plan.h"

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

int main()
{
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
