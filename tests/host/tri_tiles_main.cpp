// The tile decode of the agreement and co-association kernels (csrc/mi_tri_tiles.h) as a host program.  For every nb in
// [1, small] (argv[1], default 400) every tile number q is decoded and compared with the pair a plain double loop over
// bi <= bj reaches at position q; for every further nb on the command line (default 782 1024 4096 16384 65536) the first
// and the last q of every tile row (bj = bi and bj = nb - 1) and q = tpg - 1.  Prints the first mismatch and exits 1;
// otherwise prints the number of decodes checked.  tests/test_tri_tiles_host.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../scrna_seq_qannealing_clustering_amd/csrc/mi_tri_tiles.h"

static long long checked = 0;

static bool check(int nb, long long q, int want_bi, int want_bj)
{
    int bi = -1, bj = -1;
    mi_tri::tile_of(q, nb, &bi, &bj);
    ++checked;
    if (bi == want_bi && bj == want_bj) return true;
    std::printf("mismatch: nb = %d, q = %lld: decoded (%d, %d), the double loop gives (%d, %d)\n", nb, q, bi, bj, want_bi, want_bj);
    return false;
}

int main(int argc, char **argv)
{
    const int small = argc > 1 ? std::atoi(argv[1]) : 400;
    std::vector<int> large;
    for (int a = 2; a < argc; ++a) large.push_back(std::atoi(argv[a]));
    if (argc <= 2) large = {782, 1024, 4096, 16384, 65536};
    if (small < 1) return 2;
    for (int nb = 1; nb <= small; ++nb) {
        long long q = 0;
        for (int bi = 0; bi < nb; ++bi)
            for (int bj = bi; bj < nb; ++bj, ++q)
                if (!check(nb, q, bi, bj)) return 1;
        if (q != (long long)nb * (nb + 1) / 2) return 2;
    }
    for (int nb : large) {
        if (nb < 1 || nb > 65536) return 2;
        long long start = 0;                                      // of tile row bi, counted row by row
        for (int bi = 0; bi < nb; ++bi) {
            if (!check(nb, start, bi, bi)) return 1;
            start += nb - bi;
            if (!check(nb, start - 1, bi, nb - 1)) return 1;
        }
        const long long tpg = (long long)nb * (nb + 1) / 2;
        if (start != tpg) return 2;
        if (!check(nb, tpg - 1, nb - 1, nb - 1)) return 1;
    }
    std::printf("ok %lld\n", checked);
    return 0;
}
