// cusp/precond/aggregation/smooth_prolongator.h -- smooth_prolongator(S, T, P, rho_Dinv_S = 0, omega = 4/3):
//   P = T - (omega / rho) D^-1 S T        (reference cusp/precond/aggregation/smooth_prolongator.h)
// in the order of the reference's sequential path (system/detail/sequential/smooth_prolongator.h): every value of S is divided by its
// row's diagonal and then multiplied by lambda = omega / rho; cusp::multiply(D_inv_S, T, temp); cusp::subtract(T, temp, P).
// rho_Dinv_S == 0 means "estimate it with cusp::eigen::estimate_rho_Dinv_A(S)".
//   host_memory   : those loops.   device_memory : cmi_csr_scale_rows_*, then the device SpGEMM and cmi_csr_elementwise_*.
// The device product keeps exact-zero sums that the host product drops; the subtraction drops what cancels
// and keeps T's entry otherwise, so P has the host path's bits either way.
// Not built: the fused kernel for one entry of T per row.
#pragma once
#include "../../eigen/spectral_radius.h"
#include "../../elementwise.h"
#include "../../format_utils.h"
#include "../../multiply.h"

namespace cusp {
namespace precond {
namespace aggregation {
namespace detail {

template <typename M, typename D, typename V> void scale_rows(M &m, const D &d, V lambda, cusp::host_memory)
{
    for (size_t i = 0; i < m.num_rows; i++)
        for (auto q = m.row_offsets[i]; q < m.row_offsets[i + 1]; q++) {
            const V quotient = V(m.values[q]) / V(d[i]);
            m.values[q] = quotient * lambda;
        }
}
template <typename M, typename D, typename V> void scale_rows(M &m, const D &d, V lambda, cusp::device_memory)
{
    cusp::detail::check(cusp::detail::by_type<typename M::value_type>(cmi_csr_scale_rows_f64, cmi_csr_scale_rows_f32)(
        (int64_t)m.num_rows, (int64_t)m.num_entries, m.row_offsets.data(), m.values.data(), d.data(), lambda,
                                                                                                                      m.values.data(), nullptr)); // in place: the values are input and output
}

} // namespace detail

template <typename MatrixType1, typename MatrixType2, typename MatrixType3>
void smooth_prolongator(const MatrixType1 &S, const MatrixType2 &T, MatrixType3 &P, double rho_Dinv_S = 0.0, const double omega = 4.0 / 3.0)
{
    typedef typename MatrixType3::index_type I;
    typedef typename MatrixType3::value_type V;
    typedef typename MatrixType3::memory_space Space;
    static_assert(std::is_same<typename MatrixType1::format, cusp::csr_format>::value && std::is_same<typename MatrixType2::format, cusp::csr_format>::value &&
                      std::is_same<typename MatrixType3::format, cusp::csr_format>::value,
                  "smooth_prolongator is implemented for csr matrices: cusp::convert first");
    if (rho_Dinv_S == 0.0) rho_Dinv_S = cusp::eigen::estimate_rho_Dinv_A(S);
    cusp::array1d<V, Space> D;
    cusp::extract_diagonal(S, D);
    cusp::csr_matrix<I, V, Space> D_inv_S(S), temp;
    const V lambda = static_cast<V>(omega / rho_Dinv_S);
    detail::scale_rows(D_inv_S, D, lambda, Space());
    cusp::multiply(D_inv_S, T, temp);
    cusp::subtract(T, temp, P);
}

} // namespace aggregation
} // namespace precond
} // namespace cusp
