// mi_prep_handle.h -- the definition of mi_prep_matrix (include/mi_prep.h), shared by the translation units that serve the
// handle: prep_kernels.hip (every preprocessing pass) and markers_kernels.hip (mi_prep_rank_sum_markers), and the one way
// into their entry points.  Internal.
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

namespace mi_sa_impl {

// what an entry needs of the handle's state: mi_prep_normalize has run, a selection (mi_prep_select*) has run
enum : unsigned { NEED_NORMALIZED = 1, NEED_SELECTED = 2 };

inline int check_state(const mi_prep_matrix *m, unsigned need)
{
    if ((need & NEED_NORMALIZED) && !m->normalized) return fail(MI_ESTATE, "mi_prep_normalize has not run");
    if ((need & NEED_SELECTED) && m->h < 1) return fail(MI_ESTATE, "mi_prep_select has not run");
    return MI_OK;
}

// The one way into an entry point on a handle, always in this order: *out_kernel_ms is zeroed; no exception leaves it; the
// handle (and, where the entry has other pointer arguments that must be given, args_ok) is not null; the handle is in the
// state `need` asks for; its device is current.  The handle's state is the body's business: an entry that checks a range
// before the state passes need = 0 and calls check_state where its order has it.
template <typename F>
int on_matrix(mi_prep_matrix *m, bool args_ok, unsigned need, float *out_kernel_ms, F &&body)
{
    if (out_kernel_ms) *out_kernel_ms = 0.0f;
    return guarded([&]() -> int {
        if (!m || !args_ok) return fail(MI_EINVAL, "NULL argument");
        MI_TRY(check_state(m, need));
        HIP_TRY(hipSetDevice(m->device));
        return body();
    });
}

}  // namespace mi_sa_impl
