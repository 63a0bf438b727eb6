// cusp/krylov/detail/multiply_dot.h -- y <- A v and *out <- <y, w> for the fused solvers on device_memory (cg, cg with the Jacobi preconditioner,
// cr, cg_m): ONE ladder for float and double.  A format whose kernel can fold the dot into the multiply does so in one launch
// (cmi_spmv_*_dot_*); everything else multiplies and then runs the dot.  The scalar is a double in device memory for both value types (float
// vectors: cmi_blas_dotd_f32 accumulates in double).
#pragma once
#include <type_traits>

#include "../../multiply.h"

namespace cusp {
namespace krylov {
namespace detail {

using cusp::detail::by_type;

// the two-launch route: cusp::multiply (a format's kernel through the container's plan, or the operator's own operator()), then the dot
template <typename A, typename V> void multiply_then_dot(const A &a, const V &v, V &y, const V &w, double *out, void *ws)
{
    typedef typename A::value_type T;
    cusp::multiply(a, v, y);
    cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(y.size(), y.data(), w.data(), out, ws, nullptr));
}

template <typename A, typename V> void multiply_dot(const A &a, const V &v, V &y, const V &w, double *out, void *ws)
{
    using cusp::detail::check;
    using cusp::detail::data_of;
    using cusp::detail::forced_config;
    using cusp::detail::plan_of;
    typedef typename A::value_type T;
    if constexpr (!cusp::detail::has_format<A>::value) { // a linear operator without a format
        multiply_then_dot(a, v, y, w, out, ws);
    } else {
        typedef typename A::format Format;
        // every operator with a format, both value types: the sizes are checked here, before any entry point sees them
        if (v.size() != a.num_cols || y.size() != a.num_rows) throw cusp::invalid_input_exception("cg: vector sizes do not match the matrix");
        if constexpr (std::is_same<Format, cusp::csr_format>::value) { // steered by the container's plan where there is one
            cusp::detail::require_int_index<A>();
            if (const cmi_plan *pl = plan_of(a, nullptr, 0))
                check(by_type<T>(cmi_spmv_csr_dot_plan_f64, cmi_spmv_csr_dot_plan_f32)(pl, a.row_offsets.data(), a.column_indices.data(), a.values.data(), v.data(), y.data(),
                                                                                       w.data(), out, ws, nullptr));
            else
                check(by_type<T>(cmi_spmv_csr_dot_f64, cmi_spmv_csr_dot_f32)(a.num_rows, a.num_cols, a.num_entries, a.row_offsets.data(), a.column_indices.data(), a.values.data(),
                                                                             v.data(), y.data(), w.data(), out, ws, forced_config(), nullptr));
        } else if constexpr (std::is_same<Format, cusp::ell_format>::value) {
            cusp::detail::require_int_index<A>();
            check(by_type<T>(cmi_spmv_ell_dot_f64, cmi_spmv_ell_dot_f32)(a.num_rows, a.num_cols, a.column_indices.num_cols, a.column_indices.pitch, data_of(a.column_indices),
                                                                         data_of(a.values), cusp::detail::row_lengths_of(a, 0), v.data(), y.data(), w.data(), out, ws,
                                                                         forced_config(), nullptr));
        } else if constexpr (std::is_same<Format, cusp::dia_format>::value) {
            cusp::detail::require_int_index<A>();
            check(by_type<T>(cmi_spmv_dia_dot_f64, cmi_spmv_dia_dot_f32)(a.num_rows, a.num_cols, a.values.num_cols, a.values.pitch, a.diagonal_offsets.data(), data_of(a.values),
                                                                         v.data(), y.data(), w.data(), out, ws, forced_config(), nullptr));
        } else if constexpr (std::is_same<Format, cusp::coo_format>::value) { // through its plan: sorted entries run the CSR kernel's fused dot on the plan's row offsets
            cusp::detail::require_int_index<A>();
            if (const cmi_plan *pl = plan_of(a, nullptr, 0))
                check(by_type<T>(cmi_spmv_coo_dot_plan_f64, cmi_spmv_coo_dot_plan_f32)(pl, a.row_indices.data(), a.column_indices.data(), a.values.data(), v.data(), y.data(),
                                                                                       w.data(), out, ws, nullptr));
            else
                multiply_then_dot(a, v, y, w, out, ws);
        } else if constexpr (std::is_same<Format, cusp::hyb_format>::value) {
            cusp::detail::require_int_index<A>();
            const bool one_pitch = a.ell.column_indices.pitch == a.ell.values.pitch;
            // an empty COO part (the tuned width rule keeps regular matrices entirely in the ELL part): the ELL kernel's fused dot -- double only, float keeps the plan route
            if constexpr (std::is_same<T, double>::value)
                if (a.coo.num_entries == 0 && one_pitch) return multiply_dot(a.ell, v, y, w, out, ws);
            // one launch through the plan, which takes ONE pitch for both ELL arrays: guarded for both value types
            if (const cmi_plan *pl = one_pitch ? plan_of(a, nullptr, 0) : nullptr)
                check(by_type<T>(cmi_spmv_hyb_dot_plan_f64, cmi_spmv_hyb_dot_plan_f32)(pl, a.ell.column_indices.pitch, data_of(a.ell.column_indices), data_of(a.ell.values),
                                                                                       a.coo.row_indices.data(), a.coo.column_indices.data(), a.coo.values.data(), v.data(),
                                                                                       y.data(), w.data(), out, ws, nullptr));
            else
                multiply_then_dot(a, v, y, w, out, ws);
        } else {
            multiply_then_dot(a, v, y, w, out, ws);
        }
    }
}

} // namespace detail
} // namespace krylov
} // namespace cusp
