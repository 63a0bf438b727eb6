// cusp/detail/config.h -- glue between the header-only cusp:: layer and the C-ABI library
// (include/cusp_mi355x.h).  Every C-ABI status becomes the cusp exception the reference would throw
// for the same condition (cusp/exception.h); unlike the reference, kernel-launch failures are reported.
#pragma once
#include <cstdlib>
#include <new>
#include <string>
#include <type_traits>

#include "../../../../include/cusp_mi355x.h"
#include "../exception.h"

#define CUSP_MI355X 1
#define CUSP_VERSION 500 /* API level of the reference this layer mirrors: CUSP v0.5.x */

namespace cusp {
namespace detail {

inline void check(int status)
{
    if (status == CMI_SUCCESS) return;
    const std::string msg = std::string(cmi_status_string(status)) + ": " + cmi_last_error();
    switch (status) {
    case CMI_ERROR_INVALID_VALUE: throw cusp::invalid_input_exception(msg);
    case CMI_ERROR_NOT_SUPPORTED: throw cusp::not_implemented_exception(msg);
    case CMI_ERROR_ALLOC: throw std::bad_alloc();
    case CMI_ERROR_IO: throw cusp::io_exception(msg);
    default: throw cusp::runtime_exception(msg);
    }
}

// The C-ABI names its entry points by value type: by_type<T>(cmi_x_f64, cmi_x_f32) is the first for T = double and the second for T = float,
// so a call reads check(by_type<T>(cmi_blas_axpy_f64, cmi_blas_axpy_f32)(n, a, x, y, nullptr)) with both symbols at the call site.
template <typename T> struct is_real : std::integral_constant<bool, std::is_same<T, double>::value || std::is_same<T, float>::value> {};
template <typename T, typename F64, typename F32> constexpr auto by_type([[maybe_unused]] F64 *f64, [[maybe_unused]] F32 *f32)
{
    static_assert(is_real<T>::value, "the device kernels are implemented for float and double");
    if constexpr (std::is_same<T, double>::value) return f64;
    else return f32;
}

// cusp::detail::round_up (reference cusp/detail/utils.h:24-28)
template <typename I> inline I round_up(I n, I k) { return k * ((n + k - 1) / k); }

} // namespace detail
} // namespace cusp
