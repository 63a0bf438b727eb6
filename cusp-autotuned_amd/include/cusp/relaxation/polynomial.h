// cusp/relaxation/polynomial.h -- cusp::relaxation::polynomial<ValueType, MemorySpace>: the polynomial smoother
//   r = b - A x;  h = c_0 r;  h = A h + c_i r  (i = 1 .. degree - 1);  x = x + h
// (reference cusp/relaxation/polynomial.h, detail/polynomial.inl:117-142), Horner's rule on the residual.
//
//   polynomial(A, coefficients)   keeps all but the LAST coefficient, negated, as default_coefficients (polynomial.inl:
//                                 92-98: a polynomial normalised to constant term 1, as chebyshev_polynomial_coefficients
//                                 returns it, becomes the smoother's own coefficients that way).
//   relax(A, b, x)                uses default_coefficients;  relax(A, b, x, coefficients) uses the given ones AS THEY ARE.
//   nrm2(x) == 0                  the residual is b itself, no multiply (polynomial.inl:119-122).
//
// NOT declared: the one-argument polynomial(A), which estimates the spectral radius with
// cusp::eigen::ritz_spectral_radius.  Using it is a compile-time error with this header: the class stays free of the
// eigensolver.  The reference constructor's recipe is the free factory of cusp/relaxation/chebyshev.h,
// make_chebyshev_polynomial<ValueType, MemorySpace>(A); with a spectral radius of your own, compute the coefficients with
// detail::chebyshev_polynomial_coefficients(rho, coefficients) and pass them to polynomial(A, coefficients).
//
//   host_memory and device_memory, all five formats: the reference's sequence through cusp::multiply and
//                   cusp::blas::axpby / axpy -- on the device the matrix's planned multiply and one elementwise launch per step.
// The one-launch form of the residual and of a degree step for CSR, cmi_spmv_csr_axpby_* (alpha = -1, beta = 1, z = b;
// alpha = 1, beta = c_i, z = residual), is in the C-ABI but NOT used here: on the 5-point Poisson matrix it measured 1.04
// (f64) and 1.27 (f32) times the two launches (profiles/r06_relax_bench.txt).  Both give the same bits.
#pragma once
#include <cmath>
#include <vector>
#include "../blas/blas.h"
#include "../linear_operator.h"
#include "../multiply.h"

namespace cusp {
namespace relaxation {

namespace detail {

// chebyshev_polynomial_coefficients(rho, coefficients, lower_bound = 1/30, upper_bound = 1.1): the cubic whose roots are the
// three Chebyshev points of the interval [lower_bound * rho, upper_bound * rho], normalised to constant term 1; four
// coefficients, highest power first (the reference's function of this name, polynomial.inl).  Host arithmetic only.  The
// monic product (t - r_0)(t - r_1)(t - r_2) is built one linear factor at a time.
template <typename ValueType>
void chebyshev_polynomial_coefficients(const ValueType rho, cusp::array1d<ValueType, cusp::host_memory> &coefficients,
                                       const ValueType lower_bound = ValueType(1.0 / 30.0), const ValueType upper_bound = ValueType(1.1))
{
    const int points = 3;
    const double pi = 3.14159265358979323846;
    const ValueType lo = lower_bound * rho, width = upper_bound * rho - lo;
    std::vector<ValueType> poly(1, ValueType(1));
    for (int k = 0; k < points; k++) {
        const ValueType t = ValueType(std::cos(pi * (2 * k + 1) / (2 * points))); // Chebyshev point of [-1, 1]
        const ValueType root = lo + width * (t + 1) / 2;
        poly.push_back(ValueType(0));                                             // poly <- poly * (t - root)
        for (size_t j = poly.size() - 1; j > 0; j--) poly[j] = poly[j] - root * poly[j - 1];
    }
    coefficients.resize(poly.size());
    for (size_t j = 0; j < poly.size(); j++) coefficients[j] = poly[j] / poly.back();
}

} // namespace detail

template <typename ValueType, typename MemorySpace> class polynomial : public cusp::linear_operator<ValueType, MemorySpace> {
    typedef cusp::linear_operator<ValueType, MemorySpace> Parent;

public:
    cusp::array1d<ValueType, cusp::host_memory> default_coefficients; // on the host: they are launch arguments
    cusp::array1d<ValueType, MemorySpace> residual;
    cusp::array1d<ValueType, MemorySpace> h;
    cusp::array1d<ValueType, MemorySpace> y;

    polynomial() {}

    template <typename MatrixType, typename VectorType>
    polynomial(const MatrixType &A, const VectorType &coefficients)
        : Parent(A.num_rows, A.num_cols, A.num_entries), residual(A.num_rows, ValueType(0)), h(A.num_rows, ValueType(0)), y(A.num_rows, ValueType(0))
    {
        if (coefficients.size() == 0) throw cusp::invalid_input_exception("cusp::relaxation::polynomial: no coefficients");
        const size_t kept = coefficients.size() - 1;
        default_coefficients.resize(kept);
        for (size_t i = 0; i < kept; i++) default_coefficients[i] = -ValueType(coefficients[i]);
    }

    template <typename MemorySpace2>
    polynomial(const polynomial<ValueType, MemorySpace2> &o)
        : Parent(o.num_rows, o.num_cols, o.num_entries), default_coefficients(o.default_coefficients), residual(o.residual), h(o.h), y(o.y) {}

    template <typename MatrixType, typename VectorType1, typename VectorType2> void operator()(const MatrixType &A, const VectorType1 &b, VectorType2 &x)
    {
        (*this)(A, b, x, default_coefficients);
    }

    template <typename MatrixType, typename VectorType1, typename VectorType2, typename VectorType3>
    void operator()(const MatrixType &A, const VectorType1 &b, VectorType2 &x, const VectorType3 &coefficients)
    {
        if (A.num_rows != A.num_cols || b.size() != A.num_rows || x.size() != A.num_rows)
            throw cusp::invalid_input_exception("cusp::relaxation::polynomial: A must be square, b and x of its size");
        if (coefficients.size() == 0) throw cusp::invalid_input_exception("cusp::relaxation::polynomial: no coefficients");
        std::vector<ValueType> c(coefficients.size());
        for (size_t i = 0; i < c.size(); i++) c[i] = ValueType(coefficients[i]);
        const size_t n = A.num_rows;
        if (residual.size() != n) residual.resize(n, ValueType(0));
        if (h.size() != n) h.resize(n, ValueType(0));
        if (y.size() != n) y.resize(n, ValueType(0));
        if (n == 0) return;

        if (cusp::blas::nrm2(x) == ValueType(0)) cusp::blas::copy(b, residual);
        else { // residual <- b - A x, as 1 * b + (-1) * (A x)
            cusp::multiply(A, x, residual);
            cusp::blas::axpby(b, residual, residual, ValueType(1), ValueType(-1));
        }
        cusp::blas::axpby(residual, h, h, c[0], ValueType(0));
        for (size_t i = 1; i < c.size(); i++) { // h <- A h + c_i residual, as 1 * (A h) + c_i * residual
            cusp::multiply(A, h, y);
            cusp::blas::axpby(y, residual, h, ValueType(1), c[i]);
        }
        cusp::blas::axpy(h, x, ValueType(1));
    }
};

} // namespace relaxation
} // namespace cusp
