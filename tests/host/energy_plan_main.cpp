// The work split of the MFMA energy kernel (csrc/mi_energy_plan.h) as a host program; the launcher and the kernel compile
// the same text.
//   energy_plan sweep              for every T in 1..48, rtiles in 1..64 and cus in {64, 104, 128, 256, 304}:
//                                  1 <= pieces <= S; the ranges [s0, s1) of the pieces are disjoint, in order and cover
//                                  [0, S) exactly; and the walk the kernel performs from s0 (block_of, then next_block
//                                  after every block) visits exactly the blocks s0 .. s1 - 1 of the row-major upper
//                                  triangle, reporting a new row exactly where there is one.  Prints the first violation
//                                  and exits 1; otherwise "ok <plans> <blocks walked>".
//   energy_plan plan n R cus ...   one line "n R cus T rtiles S pieces min_len max_len" per triple (lengths in blocks).
// tests/test_energy_plan_host.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <utility>
#include <vector>

#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_energy_plan.h"

static const int kTile = 128;

static long long walked = 0;

static bool check_plan(int T, int rtiles, int cus)
{
    const int S = (int)mi_energy_plan::blocks(T);
    const long long pieces = mi_energy_plan::pieces(T, rtiles, cus);
    if (pieces < 1 || pieces > S) {
        std::printf("T = %d, rtiles = %d, cus = %d: %lld pieces for %d blocks\n", T, rtiles, cus, pieces, S);
        return false;
    }
    std::vector<std::pair<int, int>> tri;                        // the row-major upper triangle by a plain double loop
    for (int I = 0; I < T; ++I)
        for (int K = I; K < T; ++K) tri.push_back({I, K});
    int end = 0;
    for (int piece = 0; piece < (int)pieces; ++piece) {
        int s0 = -1, s1 = -1;
        mi_energy_plan::piece_range(S, piece, (int)pieces, &s0, &s1);
        if (s0 != end || s1 <= s0 || s1 > S) {                   // (pieces <= S: no piece is empty)
            std::printf("T = %d, rtiles = %d, cus = %d: piece %d of %lld is [%d, %d) after %d\n", T, rtiles, cus, piece, pieces, s0, s1, end);
            return false;
        }
        end = s1;
        int cI = -1, cK = -1;
        mi_energy_plan::block_of(s0, T, &cI, &cK);
        for (int s = s0; s < s1; ++s) {
            if (cI != tri[s].first || cK != tri[s].second) {
                std::printf("T = %d, piece [%d, %d): block %d walked as (%d, %d), the double loop gives (%d, %d)\n", T, s0, s1, s, cI,
                            cK, tri[s].first, tri[s].second);
                return false;
            }
            const bool last_of_row = cK == T - 1;
            if (mi_energy_plan::next_block(T, &cI, &cK) != last_of_row) {
                std::printf("T = %d: the step after block %d reports the wrong row change\n", T, s);
                return false;
            }
            ++walked;
        }
    }
    if (end != S) {
        std::printf("T = %d, rtiles = %d, cus = %d: the pieces end at %d of %d\n", T, rtiles, cus, end, S);
        return false;
    }
    return true;
}

int main(int argc, char **argv)
{
    if (argc == 2 && !std::strcmp(argv[1], "sweep")) {
        const int cus_list[] = {64, 104, 128, 256, 304};
        long long plans = 0;
        for (int cus : cus_list)
            for (int T = 1; T <= 48; ++T)
                for (int rtiles = 1; rtiles <= 64; ++rtiles, ++plans)
                    if (!check_plan(T, rtiles, cus)) return 1;
        std::printf("ok %lld %lld\n", plans, walked);
        return 0;
    }
    if (argc < 5 || std::strcmp(argv[1], "plan") || (argc - 2) % 3) return 2;
    for (int a = 2; a + 2 < argc; a += 3) {
        const int n = std::atoi(argv[a]), R = std::atoi(argv[a + 1]), cus = std::atoi(argv[a + 2]);
        if (n < 1 || R < 1 || cus < 1) return 2;
        const int T = (n + kTile - 1) / kTile, rtiles = (R + kTile - 1) / kTile, S = (int)mi_energy_plan::blocks(T);
        const int pieces = (int)mi_energy_plan::pieces(T, rtiles, cus);
        int lo = S, hi = 0;
        for (int piece = 0; piece < pieces; ++piece) {
            int s0, s1;
            mi_energy_plan::piece_range(S, piece, pieces, &s0, &s1);
            lo = s1 - s0 < lo ? s1 - s0 : lo;
            hi = s1 - s0 > hi ? s1 - s0 : hi;
        }
        std::printf("%d %d %d %d %d %d %d %d %d\n", n, R, cus, T, rtiles, S, pieces, lo, hi);
    }
    return 0;
}
