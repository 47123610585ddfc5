// mi_tri_tiles.h -- the tiles on or above the diagonal of an nb x nb block grid, numbered row by row: tile q of
// [0, nb (nb + 1) / 2) -> (bi, bj) with bi <= bj.  Tile row bi holds the nb - bi tiles bj = bi .. nb - 1 and starts at
// f(bi) = bi nb - bi (bi - 1) / 2, so bi is the largest row with f(bi) <= q: the smaller root of f(x) = q in fp64 as a
// guess (its rounding is worth a row at most where the rows are short, near bi = nb - 1), then two loops that move the
// guess onto the row exactly in int64.  k_agree_mfma (csrc/agreement_kernels.hip) and k_coassoc_mfma
// (csrc/coassoc_kernels.hip) walk their tiles with it; nb is at most 65 536 there, q up to 2.1e9.  Plain C++: the device
// code and a host program (tests/host/tri_tiles_main.cpp) compile the same text.
#pragma once

#include <math.h>

#if defined(__HIPCC__)
#define MI_TRI_FN __host__ __device__ __forceinline__
#else
#define MI_TRI_FN inline
#endif

namespace mi_tri {

// first tile of tile row x
MI_TRI_FN long long row_start(int x, int nb) { return (long long)x * nb - (long long)x * (x - 1) / 2; }

MI_TRI_FN void tile_of(long long q, int nb, int *out_bi, int *out_bj)
{
    const double b2 = 2.0 * nb + 1.0;
    int bi = (int)floor((b2 - sqrt(b2 * b2 - 8.0 * (double)q)) * 0.5);
    bi = bi < 0 ? 0 : (bi > nb - 1 ? nb - 1 : bi);
    while (bi > 0 && row_start(bi, nb) > q) --bi;
    while (bi + 1 < nb && row_start(bi + 1, nb) <= q) ++bi;
    *out_bi = bi;
    *out_bj = bi + (int)(q - row_start(bi, nb));
}

}  // namespace mi_tri
