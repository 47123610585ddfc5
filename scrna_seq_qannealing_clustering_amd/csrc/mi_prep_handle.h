// mi_prep_handle.h -- the definition of mi_prep_matrix (include/mi_prep.h), shared by the translation units that serve the
// handle: prep_kernels.hip (every preprocessing pass) and markers_kernels.hip (mi_prep_rank_sum_markers).  Internal.
#pragma once

#include <cstdint>

#include "mi_sa_host.h"

struct mi_prep_matrix {
    int n = 0, g = 0, device = 0, h = 0, ldz = 0;
    bool normalized = false, sparse = false;
    int64_t nnz = 0;                                              // stored entries of a sparse handle
    mi_sa_impl::DevArray<float> d_X, d_Y, d_Z;                    // sparse: d_X, d_Y hold nnz values in the caller's CSR order
    mi_sa_impl::DevArray<int64_t> d_indptr, d_colptr;             // sparse: the caller's CSR structure and its transpose,
    mi_sa_impl::DevArray<int32_t> d_indices, d_rows, d_pos;       // whose entry k is entry d_pos[k] of the CSR order
};
