// cusp/precond/aggregation/galerkin_product.h -- galerkin_product(R, A, P, RAP): RAP = R (A P), two sparse products through
// cusp::multiply (reference cusp/precond/aggregation/galerkin_product.h).
//   host_memory   : the host product drops sums that compare equal to zero, as the reference's host loop does.
//   device_memory : the device product keeps them, so each product is followed by cusp::add with an empty matrix --
//                   cmi_csr_elementwise_*, which copies a lone entry unchanged and drops what equals zero: A P and R (A P) then
//                   have the host path's structure and bits (a kept zero in A P would otherwise meet an Inf of R as a NaN).
// A product wider than SpGEMM's workspace surfaces its NOT_SUPPORTED message unchanged.
#pragma once
#include "../../elementwise.h"
#include "../../multiply.h"

namespace cusp {
namespace precond {
namespace aggregation {
namespace detail {

template <typename M> void drop_zeros(M &, cusp::host_memory) {}
template <typename M> void drop_zeros(M &m, cusp::device_memory)
{
    cusp::csr_matrix<typename M::index_type, typename M::value_type, cusp::host_memory> none(m.num_rows, m.num_cols, 0);
    for (size_t i = 0; i <= m.num_rows; i++) none.row_offsets[i] = 0;
    M empty(none), out;
    cusp::add(m, empty, out);
    m.swap(out);
}

} // namespace detail

template <typename MatrixType1, typename MatrixType2, typename MatrixType3, typename MatrixType4>
void galerkin_product(const MatrixType1 &R, const MatrixType2 &A, const MatrixType3 &P, MatrixType4 &RAP)
{
    static_assert(std::is_same<typename MatrixType4::format, cusp::csr_format>::value, "galerkin_product writes a csr matrix");
    MatrixType4 AP;
    cusp::multiply(A, P, AP);
    detail::drop_zeros(AP, typename MatrixType4::memory_space());
    cusp::multiply(R, AP, RAP);
    detail::drop_zeros(RAP, typename MatrixType4::memory_space());
}

} // namespace aggregation
} // namespace precond
} // namespace cusp
