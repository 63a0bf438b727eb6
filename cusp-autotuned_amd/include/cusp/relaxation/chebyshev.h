// cusp/relaxation/chebyshev.h -- cusp::relaxation::make_chebyshev_polynomial<ValueType, MemorySpace>(A): the polynomial smoother
// with the coefficients the reference's one-argument constructor polynomial(A) computes (reference detail/polynomial.inl):
//   rho = cusp::eigen::ritz_spectral_radius(A, 8, true);  chebyshev_polynomial_coefficients(rho, c);  polynomial(A, c)
// A free function, so that cusp/relaxation/polynomial.h needs no eigensolver and polynomial(A) stays a compile-time error
// there.  A: any of the five formats in MemorySpace; on device_memory the estimate runs the fused Lanczos steps of
// cusp/eigen/arnoldi.h (one host read per step).
#pragma once
#include "../eigen/spectral_radius.h"
#include "polynomial.h"

namespace cusp {
namespace relaxation {

template <typename ValueType, typename MemorySpace, typename MatrixType> polynomial<ValueType, MemorySpace> make_chebyshev_polynomial(const MatrixType &A)
{
    const ValueType rho = static_cast<ValueType>(cusp::eigen::ritz_spectral_radius(A, 8, true));
    cusp::array1d<ValueType, cusp::host_memory> coefficients;
    detail::chebyshev_polynomial_coefficients(rho, coefficients);
    return polynomial<ValueType, MemorySpace>(A, coefficients);
}

} // namespace relaxation
} // namespace cusp
