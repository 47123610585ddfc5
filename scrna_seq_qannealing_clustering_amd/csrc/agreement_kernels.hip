// agreement_kernels.hip -- label agreement (ARI, NMI) between labellings on the i8 matrix cores (gfx950).
// C ABI: include/mi_metrics.h (mi_label_agreement_u16) and mi_sa_problem_label_agreement (include/mi_sa.h, mi_sa.hip).
//
// The contingency table of labellings a and b over n cells is onehot(a)^T onehot(b): a product of 0/1 matrices with
// the cells as the inner dimension, exact on v_mfma_i32_16x16x64_i8 (i8 products, i32 accumulate).  Nothing R K x R K
// is materialised: every pair's table lives in the accumulators of one wavefront and is reduced there.
//
//   k_xlogx        tab[v] = v ln v for v = 0 .. n (every entropy term below reads it: one log per value, shared)
//   k_agree_prep   one workgroup per labelling: uint16 labels -> one byte per cell (holes and padding: 0x7F), and
//                  the labelling's cluster sizes a_c -> sum C(a_c, 2) (int64), sum a_c ln a_c, non-empty clusters
//   k_agree_mfma   one wavefront per tile of T x T labellings (T = 4 / KB; K padded to 16 KB labels, KB = 1, 2, 4):
//                  per chunk of 64 cells it builds the 2 T KB one-hot fragments in registers and issues T^2 KB^2 MFMAs
//                  (16 per chunk at every K); then per pair S = sum C(n_ij, 2) in int64, T = sum n_ij ln n_ij in fp64
//                  (fixed order: the lane's entries, then a butterfly over the lanes) and the closed forms in fp64.
//
// Operand maps of v_mfma_i32_16x16x64_i8 as used here: lane l holds A[row l & 15][16 cells of lane group l >> 4] and
// B[the same 16 cells][col l & 15], 16 bytes each; register q of the accumulator is C[row 4 (l >> 4) + q][col l & 15]
// (the C/D map of every 16x16 form).  The order of the cells inside a k-step is irrelevant to a contingency table as
// long as both operands put the same cell at the same (lane group, byte): they are built from the same cell offsets.
// The tests pin the map with asymmetric data (Ka != Kb, A != B, exact tables).
//
// The one-hot fragment of label row c from four label bytes w: x = w ^ c * 0x01010101 has a zero byte exactly where
// the label is c; every byte of x is < 0x80 (labels and c < 64, padding 0x7F), so x + 0x7F7F7F7F carries out of no
// byte and its bit 7 is clear exactly at the zero bytes.  All of it is vector work of the wavefront that issues the
// MFMAs (vector instructions do not issue beside MFMA-streaming waves of the same SIMD, so no
// SIMD mate does it): one wavefront per SIMD, a persistent loop over tiles, loads two chunks ahead.  In WITHIN mode the
// tiles on or above the diagonal are numbered row by row; mi_tri_tiles.h turns a tile's number into (bi, bj), the same
// text as in coassoc_kernels.hip and in the host program that checks it (tests/host/tri_tiles_main.cpp).
#include <cmath>
#include <vector>

#include "../../include/mi_metrics.h"
#include "mi_sa_device.h"
#include "mi_tri_tiles.h"

namespace mi_sa_impl {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr unsigned kPadLabel = 0x7Fu;      // holes and cells past n: matches no label row
constexpr int kAgreeWaves = 4;             // wavefronts per workgroup, each on its own tiles

__global__ void __launch_bounds__(256) k_xlogx(int n, double *__restrict__ tab)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v <= n) tab[v] = v > 1 ? (double)v * log((double)v) : 0.0;
}

// labelling r = row r of L (row stride ld, columns [0, cols)); column i is skipped when meta && meta[i] >> 31 (a hole seat
// of the padded Potts layout)
__global__ void __launch_bounds__(256) k_agree_prep(const uint16_t *__restrict__ L, size_t ld, int cols,
                                                    const uint32_t *__restrict__ meta, int npad, const double *__restrict__ tab,
                                                    uint8_t *__restrict__ lab8, long long *__restrict__ st_s,
                                                    double *__restrict__ st_t, int *__restrict__ st_k)
{
    __shared__ int hist[64];
    const int r = blockIdx.x, tid = threadIdx.x;
    if (tid < 64) hist[tid] = 0;
    __syncthreads();
    const uint16_t *row = L + (size_t)r * ld;
    uint8_t *out = lab8 + (size_t)r * npad;
    for (int i = tid; i < npad; i += 256) {
        unsigned v = kPadLabel;
        if (i < cols && !(meta && (meta[i] >> 31))) {
            const unsigned l = row[i];
            if (l < 64u) { v = l; atomicAdd(&hist[l], 1); }            // (labels are validated < K <= 64 by the callers)
        }
        out[i] = (uint8_t)v;
    }
    __syncthreads();
    if (tid < 64) {
        const int c = hist[tid];
        long long s = (long long)c * (c - 1) / 2;
        double t = tab[c];
        int k = c > 0 ? 1 : 0;
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            s += __shfl_xor(s, o, 64);
            t += __shfl_xor(t, o, 64);
            k += __shfl_xor(k, o, 64);
        }
        if (tid == 0) { st_s[r] = s; st_t[r] = t; st_k[r] = k; }
    }
}

__device__ __forceinline__ unsigned onehot4(unsigned w, unsigned key)
{
    const unsigned x = w ^ key;
    return (~(x + 0x7F7F7F7Fu) >> 7) & 0x01010101u;
}

// ARI (Hubert-Arabie) and NMI (arithmetic normalisation) of one pair from its integer sums; sklearn's special cases
__device__ __forceinline__ void agree_closed_forms(long long S, double T, long long a, double ta, int ka, long long b,
                                                   double tb, int kb, int n, double *ari, double *nmi)
{
    const double N = (double)n, C2 = 0.5 * N * (N - 1.0);
    if (S == a && S == b) {
        *ari = 1.0;                                           // no pair split by one labelling and joined by the other
    } else {
        const double p = (double)a * (double)b / C2;
        const double den = 0.5 * ((double)a + (double)b) - p;
        *ari = den == 0.0 ? 1.0 : ((double)S - p) / den;
    }
    if (ka == 1 && kb == 1) {
        *nmi = 1.0;
    } else if (ka == 1 || kb == 1) {
        *nmi = 0.0;
    } else {
        const double lnN = log(N);
        double mi = (T - ta - tb) / N + lnN;
        mi = mi > 0.0 ? mi : 0.0;
        const double ha = lnN - ta / N, hb = lnN - tb / N;
        *nmi = mi == 0.0 ? 0.0 : mi / (0.5 * (ha + hb));
    }
}

struct AgreeDev {
    const uint8_t *labA, *labB;            // one byte per cell, rows of npad bytes
    int npad, Ra, Rb;                      // CROSS: Ra x Rb pairs; WITHIN (labB == labA): Rg = Ra / groups rows per group
    int within, Rg, nbj;                   // tiles: CROSS nbj per tile row; WITHIN tpg = nb (nb + 1) / 2 per group, nb = nbj
    long long tpg, tiles;
    int n, Ka, Kb;
    const double *tab;
    const long long *sA, *sB;
    const double *tA, *tB;
    const int *kA, *kB;
    double *ari, *nmi;
    long long *S;
    int *tables;                           // CROSS only, nullable: Ka x Kb per pair
};

template <int KB, int T>
__global__ void __launch_bounds__(256) k_agree_mfma(AgreeDev g)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int grp = lane >> 4, row16 = lane & 15;
    unsigned key[KB];
#pragma unroll
    for (int rb = 0; rb < KB; ++rb) key[rb] = (unsigned)(row16 + 16 * rb) * 0x01010101u;
    const int nch = g.npad >> 6;
    for (long long w = (long long)blockIdx.x * kAgreeWaves + wave; w < g.tiles; w += (long long)gridDim.x * kAgreeWaves) {
        // tile -> (group, tile row bi, tile column bj); every value here is wave-uniform
        int base = 0, bi, bj, rowsA, rowsB;
        if (g.within) {
            const int grpi = (int)(w / g.tpg);
            const long long q = w - (long long)grpi * g.tpg;
            mi_tri::tile_of(q, g.nbj, &bi, &bj);               // tiles on or above the diagonal, row by row (mi_tri_tiles.h)
            base = grpi * g.Rg;
            rowsA = rowsB = g.Rg;
        } else {
            bi = (int)(w / g.nbj);
            bj = (int)(w - (long long)bi * g.nbj);
            rowsA = g.Ra;
            rowsB = g.Rb;
        }
        const uint8_t *pa[T], *pb[T];
#pragma unroll
        for (int t = 0; t < T; ++t) {
            const int ia = bi * T + t < rowsA ? bi * T + t : rowsA - 1;       // rows past the end: a valid row, result dropped
            const int ib = bj * T + t < rowsB ? bj * T + t : rowsB - 1;
            pa[t] = g.labA + (size_t)(base + ia) * g.npad + 16 * grp;
            pb[t] = g.labB + (size_t)(base + ib) * g.npad + 16 * grp;
        }
        i32x4 acc[T][T][KB][KB];
#pragma unroll
        for (int a = 0; a < T; ++a)
#pragma unroll
            for (int b = 0; b < T; ++b)
#pragma unroll
                for (int ra = 0; ra < KB; ++ra)
#pragma unroll
                    for (int rb = 0; rb < KB; ++rb) acc[a][b][ra][rb] = i32x4{0, 0, 0, 0};
        uint4 xa[T], xb[T], ya[T], yb[T];                  // label bytes of chunks c (x) and c + 1 (y) in flight
        auto load = [&](uint4 *da, uint4 *db, int c) {
#pragma unroll
            for (int t = 0; t < T; ++t) {
                da[t] = *reinterpret_cast<const uint4 *>(pa[t] + (size_t)c * 64);
                db[t] = *reinterpret_cast<const uint4 *>(pb[t] + (size_t)c * 64);
            }
        };
        auto step = [&](const uint4 *da, const uint4 *db) {
            i32x4 fa[T][KB], fb[T][KB];
#pragma unroll
            for (int t = 0; t < T; ++t)
#pragma unroll
                for (int r = 0; r < KB; ++r) {
                    fa[t][r] = i32x4{(int)onehot4(da[t].x, key[r]), (int)onehot4(da[t].y, key[r]),
                                     (int)onehot4(da[t].z, key[r]), (int)onehot4(da[t].w, key[r])};
                    fb[t][r] = i32x4{(int)onehot4(db[t].x, key[r]), (int)onehot4(db[t].y, key[r]),
                                     (int)onehot4(db[t].z, key[r]), (int)onehot4(db[t].w, key[r])};
                }
#pragma unroll
            for (int a = 0; a < T; ++a)
#pragma unroll
                for (int b = 0; b < T; ++b)
#pragma unroll
                    for (int ra = 0; ra < KB; ++ra)
#pragma unroll
                        for (int rb = 0; rb < KB; ++rb)
                            acc[a][b][ra][rb] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[a][ra], fb[b][rb], acc[a][b][ra][rb], 0, 0, 0);
        };
        load(xa, xb, 0);
        if (nch > 1) load(ya, yb, 1);
        for (int c = 0; c < nch; c += 2) {
            step(xa, xb);
            if (c + 2 < nch) load(xa, xb, c + 2);
            if (c + 1 < nch) {
                step(ya, yb);
                if (c + 3 < nch) load(ya, yb, c + 3);
            }
        }
        // epilogue: every pair of the tile that is wanted
#pragma unroll
        for (int a = 0; a < T; ++a)
#pragma unroll
            for (int b = 0; b < T; ++b) {
                const int li = bi * T + a, lj = bj * T + b;
                if (li >= rowsA || lj >= rowsB || (g.within && lj <= li)) continue;      // wave-uniform
                long long s = 0;
                double tt = 0.0;
#pragma unroll
                for (int ra = 0; ra < KB; ++ra)
#pragma unroll
                    for (int rb = 0; rb < KB; ++rb)
#pragma unroll
                        for (int q = 0; q < 4; ++q) {
                            const int v = acc[a][b][ra][rb][q];
                            s += (long long)v * (v - 1) / 2;
                            tt += g.tab[v];
                        }
#pragma unroll
                for (int o = 32; o >= 1; o >>= 1) {
                    s += __shfl_xor(s, o, 64);
                    tt += __shfl_xor(tt, o, 64);
                }
                long long pidx;
                if (g.within) {
                    const long long P = (long long)g.Rg * (g.Rg - 1) / 2;
                    pidx = (long long)(base / g.Rg) * P + (long long)li * g.Rg - (long long)li * (li + 1) / 2 + (lj - li - 1);
                } else {
                    pidx = (long long)li * g.Rb + lj;
                }
                if (g.tables) {
                    int *tb = g.tables + (size_t)pidx * g.Ka * g.Kb;
#pragma unroll
                    for (int ra = 0; ra < KB; ++ra)
#pragma unroll
                        for (int rb = 0; rb < KB; ++rb)
#pragma unroll
                            for (int q = 0; q < 4; ++q) {
                                const int row = 16 * ra + 4 * grp + q, col = 16 * rb + row16;
                                if (row < g.Ka && col < g.Kb) tb[row * g.Kb + col] = acc[a][b][ra][rb][q];
                            }
                }
                if (lane == 0) {
                    const int ia = base + li, jb = base + lj;
                    double ari, nmi;
                    agree_closed_forms(s, tt, g.sA[ia], g.tA[ia], g.kA[ia], g.sB[jb], g.tB[jb], g.kB[jb], g.n, &ari, &nmi);
                    g.ari[pidx] = ari;
                    g.nmi[pidx] = nmi;
                    g.S[pidx] = s;
                }
            }
    }
}

template <int KB>
void launch_agree(const AgreeDev &g, int blocks, hipStream_t st)
{
    hipLaunchKernelGGL((k_agree_mfma<KB, 4 / KB>), dim3(blocks), dim3(64 * kAgreeWaves), 0, st, g);
}

}  // namespace

int mi_label_agreement_dev(const AgreeArgs &in, hipStream_t st, double *out_ari, double *out_nmi, int64_t *out_pair_sum,
                           int32_t *out_tables, float *out_kernel_ms)
{
    const bool within = in.B == nullptr;
    const int Ra = in.Ra, Rb = within ? in.Ra : in.Rb, Ka = in.Ka, Kb = within ? in.Ka : in.Kb;
    const int Kmax = Ka > Kb ? Ka : Kb;
    const int KB = Kmax <= 16 ? 1 : (Kmax <= 32 ? 2 : 4), T = 4 / KB;
    const int npad = (in.cols + 63) / 64 * 64;
    const int G = within ? in.groups : 1, Rg = within ? Ra / G : 0;
    long long pairs, tiles, tpg = 0;
    int nbj;
    if (within) {
        pairs = (long long)G * Rg * (Rg - 1) / 2;
        nbj = (Rg + T - 1) / T;
        tpg = (long long)nbj * (nbj + 1) / 2;
        tiles = (long long)G * tpg;
    } else {
        pairs = (long long)Ra * Rb;
        nbj = (Rb + T - 1) / T;
        tiles = (long long)((Ra + T - 1) / T) * nbj;
    }
    if (out_kernel_ms) *out_kernel_ms = 0.0f;
    if (pairs == 0) return MI_OK;
    const int rows = within ? Ra : Ra + Rb;
    uint8_t *d_lab = nullptr;
    long long *d_s = nullptr, *d_S = nullptr;
    double *d_t = nullptr, *d_tab = nullptr, *d_ari = nullptr, *d_nmi = nullptr;
    int *d_k = nullptr, *d_tables = nullptr;
    return guarded([&]() -> int {
        DevBufs bufs;
        HIP_TRY(bufs.alloc(&d_lab, (size_t)rows * npad));
        HIP_TRY(bufs.alloc(&d_s, (size_t)rows));
        HIP_TRY(bufs.alloc(&d_t, (size_t)rows));
        HIP_TRY(bufs.alloc(&d_k, (size_t)rows));
        HIP_TRY(bufs.alloc(&d_tab, ((size_t)in.n_real + 1)));
        HIP_TRY(bufs.alloc(&d_ari, (size_t)pairs));
        HIP_TRY(bufs.alloc(&d_nmi, (size_t)pairs));
        HIP_TRY(bufs.alloc(&d_S, (size_t)pairs));
        if (out_tables) HIP_TRY(bufs.alloc(&d_tables, (size_t)pairs * Ka * Kb));
        Timer tm;
        MI_TRY(tm.start(st));
        hipLaunchKernelGGL(k_xlogx, dim3((unsigned)((in.n_real + 1 + 255) / 256)), dim3(256), 0, st, in.n_real, d_tab);
        hipLaunchKernelGGL(k_agree_prep, dim3((unsigned)Ra), dim3(256), 0, st, in.A, in.lda, in.cols, in.meta, npad,
                           (const double *)d_tab, d_lab, d_s, d_t, d_k);
        if (!within)
            hipLaunchKernelGGL(k_agree_prep, dim3((unsigned)Rb), dim3(256), 0, st, in.B, in.ldb, in.cols, in.meta, npad,
                               (const double *)d_tab, d_lab + (size_t)Ra * npad, d_s + Ra, d_t + Ra, d_k + Ra);
        HIP_TRY(hipGetLastError());
        AgreeDev g;
        g.labA = d_lab; g.labB = within ? d_lab : d_lab + (size_t)Ra * npad;
        g.npad = npad; g.Ra = Ra; g.Rb = Rb; g.within = within ? 1 : 0; g.Rg = Rg; g.nbj = nbj; g.tpg = tpg; g.tiles = tiles;
        g.n = in.n_real; g.Ka = Ka; g.Kb = Kb; g.tab = d_tab;
        g.sA = d_s; g.tA = d_t; g.kA = d_k;
        g.sB = within ? d_s : d_s + Ra; g.tB = within ? d_t : d_t + Ra; g.kB = within ? d_k : d_k + Ra;
        g.ari = d_ari; g.nmi = d_nmi; g.S = d_S; g.tables = d_tables;
        // one wavefront per SIMD (a persistent loop over the tiles), fewer when there are fewer tiles
        int dev = 0, cus = 256;
        (void)hipGetDevice(&dev);
        (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
        const long long need = (tiles + kAgreeWaves - 1) / kAgreeWaves;
        const int blocks = (int)(need < (long long)(cus > 0 ? cus : 256) ? need : (long long)(cus > 0 ? cus : 256));
        if (KB == 1) launch_agree<1>(g, blocks, st);
        else if (KB == 2) launch_agree<2>(g, blocks, st);
        else launch_agree<4>(g, blocks, st);
        MI_TRY(tm.stop(st, out_kernel_ms));
        if (out_ari) HIP_TRY(hipMemcpy(out_ari, d_ari, (size_t)pairs * sizeof(double), hipMemcpyDeviceToHost));
        if (out_nmi) HIP_TRY(hipMemcpy(out_nmi, d_nmi, (size_t)pairs * sizeof(double), hipMemcpyDeviceToHost));
        if (out_pair_sum) HIP_TRY(hipMemcpy(out_pair_sum, d_S, (size_t)pairs * sizeof(long long), hipMemcpyDeviceToHost));
        if (out_tables) HIP_TRY(hipMemcpy(out_tables, d_tables, (size_t)pairs * Ka * Kb * sizeof(int), hipMemcpyDeviceToHost));
        return MI_OK;
    });
}

}  // namespace mi_sa_impl
using namespace mi_sa_impl;

extern "C" int mi_label_agreement_u16(const uint16_t *A, int Ra, const uint16_t *B, int Rb, int n, int Ka, int Kb, int mode,
                                      int groups, int device, double *out_ari, double *out_nmi, int64_t *out_pair_sum,
                                      int32_t *out_tables, float *out_kernel_ms)
{
    if (!A) return fail(MI_EINVAL, "A is NULL");
    if (n < 1) return fail(MI_EINVAL, "n must be >= 1 (got %d)", n);
    if (Ra < 1 || Ra > MI_AGREE_MAX_LABELLINGS) return fail(MI_EINVAL, "Ra must be in [1, %d] (got %d)", MI_AGREE_MAX_LABELLINGS, Ra);
    if (Ka < 1 || Ka > 64) return fail(MI_EINVAL, "Ka must be in [1, 64] (got %d)", Ka);
    if (mode == MI_AGREE_CROSS) {
        if (!B) return fail(MI_EINVAL, "CROSS mode needs B");
        if (Rb < 1 || Rb > MI_AGREE_MAX_LABELLINGS) return fail(MI_EINVAL, "Rb must be in [1, %d] (got %d)", MI_AGREE_MAX_LABELLINGS, Rb);
        if (Kb < 1 || Kb > 64) return fail(MI_EINVAL, "Kb must be in [1, 64] (got %d)", Kb);
        if (groups != 1) return fail(MI_EINVAL, "CROSS mode takes groups = 1 (got %d)", groups);
        if ((double)Ra * Rb * Ka * Kb > (double)MI_AGREE_MAX_TABLE_ENTRIES && out_tables)
            return fail(MI_EUNSUPPORTED, "contingency tables of %d x %d pairs exceed %d entries", Ra, Rb, MI_AGREE_MAX_TABLE_ENTRIES);
    } else if (mode == MI_AGREE_WITHIN) {
        if (B) return fail(MI_EINVAL, "WITHIN mode takes B = NULL");
        if (groups < 1 || Ra % groups != 0) return fail(MI_EINVAL, "Ra = %d is not a multiple of groups = %d", Ra, groups);
        if (out_tables) return fail(MI_EINVAL, "contingency tables are returned in CROSS mode only");
        Kb = Ka;
        Rb = 0;
    } else {
        return fail(MI_EINVAL, "mode must be MI_AGREE_CROSS or MI_AGREE_WITHIN (got %d)", mode);
    }
    for (size_t e = 0; e < (size_t)Ra * n; ++e)
        if (A[e] >= Ka) return fail(MI_EINVAL, "label %d of A[%zu][%zu] outside [0, %d)", A[e], e / n, e % n, Ka);
    if (B)
        for (size_t e = 0; e < (size_t)Rb * n; ++e)
            if (B[e] >= Kb) return fail(MI_EINVAL, "label %d of B[%zu][%zu] outside [0, %d)", B[e], e / n, e % n, Kb);
    MI_TRY(pick_device(device));
    uint16_t *d_A = nullptr, *d_B = nullptr;
    return guarded([&]() -> int {
        DevBufs bufs;
        HIP_TRY(bufs.upload(&d_A, A, (size_t)Ra * n));
        if (B) HIP_TRY(bufs.upload(&d_B, B, (size_t)Rb * n));
        AgreeArgs a;
        a.A = d_A; a.lda = (size_t)n; a.B = d_B; a.ldb = (size_t)n;
        a.Ra = Ra; a.Rb = Rb; a.cols = n; a.Ka = Ka; a.Kb = Kb; a.groups = groups; a.meta = nullptr; a.n_real = n;
        return mi_label_agreement_dev(a, 0, out_ari, out_nmi, out_pair_sum, out_tables, out_kernel_ms);
    });
}
