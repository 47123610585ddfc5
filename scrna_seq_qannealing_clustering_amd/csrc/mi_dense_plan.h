// mi_dense_plan.h -- which kernel(s) serve an anneal of a dense model (MI_KIND_DENSE) of up to 4096 variables, in how many
// launches and with which buffers, decided in ONE place and in plain host code: the sibling of mi_sa_plan.h for the
// register-per-wave dense kernels.  (Above 4096 variables anneal_dense_xl in mi_sa.hip and the K1g launcher still decide.)  No HIP header or
// type, so this file compiles with any C++17 compiler and is tested without a GPU (mi_sa_plan_dense,
// tests/test_dense_plan.py, tests/host/plan_pack_main.cpp).
//
//   dense_ring_units   the LDS ring of K1w (units of GR rows that fit): WgCfg in dense_kernels.hip takes U and ok from it
//   plan_dense         n <= 4096: K1 / K1w / K1m / scheduled K1m + K1w, the ring unit, the cut into launches
//                      (dense_plan_step), the cached-field buffer, K1's replicas per launch, pacing
//   dense_plan_kernel_name   the string mi_sa_last_kernel_name reports for a plan
//
// A plan is a function of the call and of the handle's options alone -- never of which buffers earlier calls on the handle
// left allocated.
#pragma once

#include "mi_sa_plan.h"

namespace mi_sa_plan {

constexpr int kMaxDenseN = 64 * 64;              // register-per-wave kernels (K1, K1w, K1m)
constexpr int kMaxMfmaNT = 44;                   // K1m's LDS plan fits up to this width (n <= 2816)
constexpr int kWgWaves = 16;                     // K1w / K1m: replicas (wavefronts) per workgroup
constexpr int kDenseRingBytes = 160 * 1024 - 256;    // K1w's ring budget; the last 256 bytes hold the sweep-mode words
constexpr int kMaxChunks = 64;                   // K1: launches of co-resident replicas per anneal (one set of pacing words each)
constexpr int kCtrlModes = 8, kCtrlWords = 4096; // scheduled form: ctrl[kCtrlModes + c] = kernel of launch c
constexpr int kSchedFirstLen = 8;                // ... whose first launch is short: it calibrates the mode of the second

// ------------------------------------------------------------------------------------------------
// the options
// ------------------------------------------------------------------------------------------------
struct DensePlanOptions {
    int pace = 1;                    // sweep pacing on/off (speed only)
    int variant = 0;                 // 0 auto, 1 wave-per-replica (K1), 2 workgroup/LDS ring (K1w), 3 MFMA (K1m), 4 scheduled K1m + K1w
    int unit_rows = 0;               // K1w ring unit (rows per rendezvous): 0 auto, 2 or 4 (4 is refused where its ring does not fit LDS: n > 3328)
    int ondemand_permille = 40;      // K1w: on-demand sweeps below this acceptance (per mille); 0 = always stream
    int chunk_sweeps = 32;           // K1w/K1m: sweeps per launch of a run that is cut into launches (0 = one launch)
    int mfma_permille = 600;         // launches that accept >= this share of their proposals hand the next one to K1m (0 = never)
};

// every key of mi_sa_set_option that the dense planner reads, with the values it takes: the multiples of `step` in [lo, hi];
// pace takes any value (stored as 0 / 1)
struct DensePlanOptionKey { const char *key; int DensePlanOptions::*field; long lo, hi, step; };
inline constexpr DensePlanOptionKey kDensePlanOptionKeys[] = {
    {"pace", &DensePlanOptions::pace, LONG_MIN, LONG_MAX, 1},
    {"variant", &DensePlanOptions::variant, 0, 4, 1},
    {"unit_rows", &DensePlanOptions::unit_rows, 0, 4, 2},
    {"ondemand_permille", &DensePlanOptions::ondemand_permille, 0, 1000, 1},
    {"chunk_sweeps", &DensePlanOptions::chunk_sweeps, 0, LONG_MAX, 1},
    {"mfma_permille", &DensePlanOptions::mfma_permille, 0, 1000, 1},
};

// true: `key` is one of the dense planner's options and takes `value`
inline bool dense_plan_option_set(DensePlanOptions &o, const char *key, long value)
{
    for (const DensePlanOptionKey &k : kDensePlanOptionKeys)
        if (!strcmp(key, k.key) && value >= k.lo && value <= k.hi && value % k.step == 0) {
            o.*k.field = k.field == &DensePlanOptions::pace ? (value != 0) : (int)value;
            return true;
        }
    return false;
}

// ------------------------------------------------------------------------------------------------
// n <= 4096
// ------------------------------------------------------------------------------------------------
// K1w's LDS ring for NT field registers and units of GR rows (a row = NT * 256 bytes): the units that fit, capped so that
// (U - 2) * GR stays within the 6-bit vmcnt; 0: no ring (fewer than three units fit, or GR does not divide a slot)
constexpr int dense_ring_units(int NT, int GR)
{
    if (NT < 1 || GR < 1 || 64 % GR != 0) return 0;
    const int fit = kDenseRingBytes / (GR * NT * 256), cap = 2 + 60 / GR;
    const int U = fit < cap ? fit : cap;
    return U >= 3 ? U : 0;
}

constexpr int dense_width(int n) { return ((n + 63) / 64 + 3) / 4 * 4; }      // NT: fields per lane

struct DenseRun {
    int n = 0, R = 1, num_sweeps = 0, resync = 0;
    bool temps_per_replica = false;
    int cus = 0;                     // compute units of the device (0: 256)
    int resident_waves = 0;          // co-resident wavefronts of K1 at this width on the device (read only when K1 is the form)
};

enum DenseForm { DENSE_K1, DENSE_K1W, DENSE_K1M, DENSE_SCHEDULED };

struct DensePlan {
    DenseForm form = DENSE_K1;
    int NT = 0, unit_rows = 0;       // unit_rows: K1w's ring unit GR (0: a form without K1w)
    // the run as launches of sweeps [s0, s0 + len): first_len, then chunk_len each (dense_plan_step); K1 is never cut
    bool cut = false;                // more than one launch along the schedule: state and fields pass through HBM
    int num_sweeps = 0, first_len = 0, chunk_len = 0, steps = 1;
    int launches = 1;                // what mi_sa_last_launch_count reports (K1: its replica chunks; else the steps)
    size_t field_floats = 0;         // the cached-field buffer a cut run needs ([R][64 * NT]; 0: none)
    // K1
    int replicas_per_launch = 0;     // co-resident replicas, or more where kMaxChunks launches of those do not hold R
    bool k1_pace = false;            // pacing on and more than one sweep (K1 is never cut: the run's count is every launch's): the pacing
                                     // words are zeroed, and a launch is paced when its replicas are co-resident (dense_k1_paced)
    int resident_waves = 0;          // DenseRun::resident_waves, kept for dense_k1_paced
    // K1w
    bool wg_pace = false;            // pacing on and one workgroup per CU at most; WITHOUT the sweep count, which in a cut run is each
                                     // launch's own: the caller paces a launch of more than one sweep (DenseStep::len > 1)
    int ondemand_flips = 0;          // DenseArgs::ondemand_flips
};

struct DenseStep { int s0, len; bool first, last; };

// launch i of a plan (0 <= i < plan.steps): the sweeps it runs and whether it starts / ends the run
inline DenseStep dense_plan_step(const DensePlan &p, int i)
{
    if (!p.cut) return DenseStep{0, p.num_sweeps, true, true};
    const int s0 = i == 0 ? 0 : p.first_len + (i - 1) * p.chunk_len;
    const int want = i == 0 ? p.first_len : p.chunk_len;
    const bool last = s0 + want >= p.num_sweeps;
    return DenseStep{s0, last ? p.num_sweeps - s0 : want, i == 0, last};
}

// K1: launch c of a plan serves replicas [lo, lo + count)
inline bool dense_k1_paced(const DensePlan &p, int count) { return p.k1_pace && count <= p.resident_waves; }

// K1 serves the run (the only form that reads DenseRun::resident_waves): asked for, or the library's own choice below two
// workgroups' worth of replicas, without sweeps, and from 128 to 1024 replicas -- there a run is one chain's latency whatever
// serves it (85 ms per 200 sweeps at n = 2638 from 64 to 2048 replicas), and with at most one wavefront per SIMD the
// wave-per-replica kernel is the quicker one by 7-10 % (scripts/perf_dense_few.py); same chain, bit for bit
inline bool dense_plan_is_k1(const DenseRun &run, const DensePlanOptions &o)
{
    if (o.variant != 0) return o.variant == 1;
    return run.R < 2 * kWgWaves || run.num_sweeps <= 0 || (run.R >= 128 && run.R <= 1024);
}

inline int plan_dense(const DenseRun &run, const DensePlanOptions &o, DensePlan *out, std::string *err)
{
    if (run.n < 1) return plan_fail(err, MI_EINVAL, "n must be >= 1 (got %d)", run.n);
    if (run.n > kMaxDenseN) return plan_fail(err, MI_EUNSUPPORTED, "dense register kernels support n <= %d (got %d)", kMaxDenseN, run.n);
    DensePlan p;
    const int NT = p.NT = dense_width(run.n), R = run.R, cus = run.cus > 0 ? run.cus : 256;
    p.num_sweeps = p.first_len = p.chunk_len = run.num_sweeps;
    // a schedule longer than a chunk is cut into launches -- for the workgroup forms, from two workgroups' worth of replicas
    const bool cut = o.chunk_sweeps > 0 && run.num_sweeps > o.chunk_sweeps && o.variant != 1 && R >= 2 * kWgWaves;
    int variant = o.variant;
    if (variant == 0) {
        variant = dense_plan_is_k1(run, o) ? 1 : 2;
        // long schedules on sizes K1m is built for: let the device alternate K1m (hot) and K1w (cold)
        if (variant == 2 && NT <= kMaxMfmaNT && cut && o.mfma_permille > 0) variant = 4;
    }
    if (variant == 1) {
        if (run.resident_waves < 4) return plan_fail(err, MI_EHIP, "anneal kernel cannot be resident (occupancy 0)");
        p.form = DENSE_K1;
        p.resident_waves = p.replicas_per_launch = run.resident_waves;
        if ((R + p.replicas_per_launch - 1) / p.replicas_per_launch > kMaxChunks) p.replicas_per_launch = (R + kMaxChunks - 1) / kMaxChunks;
        p.launches = (R + p.replicas_per_launch - 1) / p.replicas_per_launch;
        p.k1_pace = o.pace && run.num_sweeps > 1;
        *out = p;
        return MI_OK;
    }
    p.form = variant == 3 ? DENSE_K1M : (variant == 4 && cut ? DENSE_SCHEDULED : DENSE_K1W);      // (scheduling needs the cut)
    if (cut) {
        p.cut = true;
        p.chunk_len = o.chunk_sweeps;
        p.first_len = p.form == DENSE_SCHEDULED && kSchedFirstLen < o.chunk_sweeps ? kSchedFirstLen : o.chunk_sweeps;
        p.steps = p.launches = 1 + (run.num_sweeps - p.first_len + p.chunk_len - 1) / p.chunk_len;
        p.field_floats = (size_t)R * NT * 64;
        if (p.form == DENSE_SCHEDULED && (run.num_sweeps + p.chunk_len - 1) / p.chunk_len + 2 > kCtrlWords - kCtrlModes)
            return plan_fail(err, MI_EINVAL, "too many chunks for the scheduler: raise chunk_sweeps");
    }
    if (p.form != DENSE_K1W && NT > kMaxMfmaNT)
        return plan_fail(err, MI_EUNSUPPORTED, "K1m is not built for NT=%d (n > %d)", NT, kMaxMfmaNT * 64);
    if (p.form != DENSE_K1M) {
        p.unit_rows = o.unit_rows ? o.unit_rows : (dense_ring_units(NT, 4) ? 4 : 2);       // 4 rows per rendezvous measured fastest
        if (p.unit_rows != 2 && p.unit_rows != 4)
            return plan_fail(err, MI_EUNSUPPORTED, "LDS ring unit of %d rows is not built for NT=%d", p.unit_rows, NT);
        if (!dense_ring_units(NT, p.unit_rows))
            return plan_fail(err, MI_EUNSUPPORTED, "LDS ring does not fit for NT=%d unit_rows=%d", NT, p.unit_rows);
        p.wg_pace = o.pace && (R + kWgWaves - 1) / kWgWaves <= cus;                        // one 160 KB workgroup per CU
        p.ondemand_flips = (int)((long long)o.ondemand_permille * run.n * kWgWaves / 1000);
    }
    *out = p;
    return MI_OK;
}

inline void dense_plan_kernel_name(const DensePlan &p, char *buf, size_t len)
{
    switch (p.form) {
    case DENSE_K1: snprintf(buf, len, "k_anneal_dense<%d>", p.NT); break;
    case DENSE_K1W: snprintf(buf, len, "k_anneal_dense_wg<%d,%d>", p.NT, p.unit_rows); break;
    case DENSE_K1M: snprintf(buf, len, "k_anneal_dense_mfma<%d>", p.NT); break;
    case DENSE_SCHEDULED: snprintf(buf, len, "k_anneal_dense_mfma<%d> + k_anneal_dense_wg<%d,%d>", p.NT, p.NT, p.unit_rows); break;
    }
}

}  // namespace mi_sa_plan
