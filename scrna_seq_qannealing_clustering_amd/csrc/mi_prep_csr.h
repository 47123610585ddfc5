// mi_prep_csr.h -- the host side of a sparse mi_prep_matrix (include/mi_prep.h): the checks of a caller's CSR arrays and
// the transpose (CSC) the per-gene kernels walk.  No HIP, no device code: plain g++ compiles it
// (tests/host/prep_csr_main.cpp runs it under the sanitizers).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

namespace mi_prep_csr {

// the values of MI_EINVAL and MI_EUNSUPPORTED (include/mi_sa.h), which this header does not include
constexpr int kOk = 0, kEinval = -1, kEunsupported = -5;

// Every check of mi_prep_create_csr_f32, in its documented order; `msg` receives the text of mi_last_error().  A stored
// zero is legal.  -> kOk, kEinval or kEunsupported.
inline int check(const int64_t *indptr, const int32_t *indices, const float *data, int n, int g, int max_cells,
                 int64_t max_nnz, char *msg, size_t msg_len)
{
    if (msg_len) msg[0] = 0;
    if (!indptr || !indices || !data) return snprintf(msg, msg_len, "NULL argument"), kEinval;
    if (n < 2) return snprintf(msg, msg_len, "n must be >= 2 (got %d)", n), kEinval;
    if (g < 1) return snprintf(msg, msg_len, "g must be >= 1 (got %d)", g), kEinval;
    if (n > max_cells) return snprintf(msg, msg_len, "%d cells exceed %d", n, max_cells), kEunsupported;
    if (indptr[0] != 0) return snprintf(msg, msg_len, "indptr[0] must be 0 (got %lld)", (long long)indptr[0]), kEinval;
    for (int i = 0; i < n; ++i)
        if (indptr[i + 1] < indptr[i]) return snprintf(msg, msg_len, "indptr decreases at row %d", i), kEinval;
    if (indptr[n] > max_nnz)
        return snprintf(msg, msg_len, "%lld stored entries exceed %lld", (long long)indptr[n], (long long)max_nnz), kEunsupported;
    for (int i = 0; i < n; ++i)
        for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
            const int32_t c = indices[e];
            if (c < 0 || c >= g) return snprintf(msg, msg_len, "row %d: column %d is outside [0, %d)", i, (int)c, g), kEinval;
            if (e > indptr[i] && c <= indices[e - 1])
                return snprintf(msg, msg_len, "row %d: columns are not strictly ascending at entry %lld", i, (long long)e), kEinval;
            if (!(data[e] >= 0.0f) || std::isinf(data[e]))
                return snprintf(msg, msg_len, "row %d, column %d: the value is NaN, infinite or negative", i, (int)c), kEinval;
        }
    return kOk;
}

// The transpose of a checked CSR structure, by one counting sort: column j owns the entries colptr[j] .. colptr[j + 1] - 1,
// rows ascending; entry k is in row `rows[k]` and is the caller's entry `pos[k]` (so one value array in the caller's
// order serves both walks; nnz < 2^31 keeps the positions 32-bit).  May throw std::bad_alloc.
inline void transpose(const int64_t *indptr, const int32_t *indices, int n, int g, std::vector<int64_t> &colptr,
                      std::vector<int32_t> &rows, std::vector<int32_t> &pos)
{
    const int64_t nnz = indptr[n];
    colptr.assign((size_t)g + 1, 0);
    rows.resize((size_t)nnz);
    pos.resize((size_t)nnz);
    for (int64_t e = 0; e < nnz; ++e) ++colptr[(size_t)indices[e] + 1];
    for (int j = 0; j < g; ++j) colptr[(size_t)j + 1] += colptr[j];
    std::vector<int64_t> cursor(colptr.begin(), colptr.end() - 1);
    for (int i = 0; i < n; ++i)                                   // rows in ascending order: every column's list ascends
        for (int64_t e = indptr[i]; e < indptr[i + 1]; ++e) {
            const int64_t k = cursor[indices[e]]++;
            rows[(size_t)k] = i;
            pos[(size_t)k] = (int32_t)e;
        }
}

}  // namespace mi_prep_csr
