// Shared by the relaxation test programs: the cases of the reference's testing/jacobi.cu and testing/polynomial.cu as
// templates over the matrix type, naive restatements of both smoothers on a host CSR matrix (one rounding per operation,
// sums in storage order), and checks of cusp::relaxation::jacobi / polynomial in any format and memory space against them
// bit for bit.  TEST_SPACE / TEST_SPACE_NAME are defined by the including program.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include <cusp/array2d.h>
#include <cusp/coo_matrix.h>
#include <cusp/csr_matrix.h>
#include <cusp/dia_matrix.h>
#include <cusp/ell_matrix.h>
#include <cusp/hyb_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/multiply.h>
#include <cusp/relaxation/jacobi.h>
#include <cusp/relaxation/polynomial.h>

#include "unittest.h"

namespace relax_check {

// seeded values in [-8, 8) with a fractional part: products and sums round, so order and contraction show in the bits
inline double seeded(uint64_t i)
{
    uint64_t z = i * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull;
    z ^= z >> 31; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 29;
    return (double)(z % 4096) / 256.0 - 8.0 + 1.0 / 3.0;
}
template <typename V> cusp::array1d<V, cusp::host_memory> seeded_vector(size_t n, uint64_t salt)
{
    cusp::array1d<V, cusp::host_memory> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (V)seeded(salt + 131 * i);
    return v;
}
// same bits; a NaN equals a NaN whatever its sign and payload (x86 and gfx950 produce different default NaNs)
template <typename A, typename B> bool bits_equal(const A &a, const B &b)
{
    typedef typename A::value_type V;
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        const V x = a[i], y = b[i];
        if (x != x && y != y) continue;
        if (std::memcmp(&x, &y, sizeof(V)) != 0) return false;
    }
    return true;
}
template <typename V> cusp::array2d<V, cusp::host_memory> dense(size_t n, std::vector<double> v)
{
    cusp::array2d<V, cusp::host_memory> a(n, n);
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++) a(i, j) = (V)v[i * n + j];
    return a;
}
// the 5-point stencil's structure with seeded values: every row has a nonzero diagonal, nothing is exact
template <typename V> cusp::csr_matrix<int, V, cusp::host_memory> seeded_stencil(size_t m, size_t n, uint64_t salt)
{
    cusp::csr_matrix<int, V, cusp::host_memory> A;
    cusp::gallery::poisson5pt(A, m, n);
    for (size_t k = 0; k < A.num_entries; k++) A.values[k] = (V)seeded(salt + 7 * k);
    return A;
}

// ---- naive restatements on a host CSR matrix ----
template <typename V> using hvec = cusp::array1d<V, cusp::host_memory>;
template <typename V> using hcsr = cusp::csr_matrix<int, V, cusp::host_memory>;

template <typename V> hvec<V> naive_multiply(const hcsr<V> &A, const hvec<V> &x)
{
    hvec<V> y(A.num_rows);
    for (size_t i = 0; i < A.num_rows; i++) {
        V acc = V(0);
        for (int jj = A.row_offsets[i]; jj < A.row_offsets[i + 1]; jj++) {
            const V p = A.values[jj] * x[A.column_indices[jj]];
            acc = acc + p;
        }
        y[i] = acc;
    }
    return y;
}
template <typename V> hvec<V> naive_diagonal(const hcsr<V> &A)
{
    hvec<V> d(A.num_rows, V(0));
    for (size_t i = 0; i < A.num_rows; i++)
        for (int jj = A.row_offsets[i]; jj < A.row_offsets[i + 1]; jj++)
            if ((size_t)A.column_indices[jj] == i) d[i] += A.values[jj];
    return d;
}
template <typename V> hvec<V> naive_jacobi(const hcsr<V> &A, const hvec<V> &b, const hvec<V> &x, V omega)
{
    const hvec<V> y = naive_multiply(A, x), d = naive_diagonal(A);
    hvec<V> out(x.size());
    for (size_t i = 0; i < x.size(); i++) {
        const V diff = b[i] - y[i];
        const V scaled = omega * diff;
        const V quot = scaled / d[i];
        out[i] = x[i] + quot;
    }
    return out;
}
// one call of the polynomial smoother with the coefficients as given; h is the object's state (read by the first step)
template <typename V> hvec<V> naive_polynomial(const hcsr<V> &A, const hvec<V> &b, const hvec<V> &x, const std::vector<V> &c, hvec<V> &h)
{
    const size_t n = x.size();
    bool zero = true; // nrm2(x) == 0: sqrt of a sum of squares is zero only if every square is
    for (size_t i = 0; i < n; i++) zero = zero && (x[i] * x[i] == V(0));
    hvec<V> r(n);
    if (zero) r = b;
    else {
        const hvec<V> y = naive_multiply(A, x);
        for (size_t i = 0; i < n; i++) { const V p = V(1) * b[i], q = V(-1) * y[i]; r[i] = p + q; }
    }
    for (size_t i = 0; i < n; i++) { const V p = c[0] * r[i], q = V(0) * h[i]; h[i] = p + q; }
    for (size_t k = 1; k < c.size(); k++) {
        const hvec<V> y = naive_multiply(A, h);
        for (size_t i = 0; i < n; i++) { const V p = V(1) * y[i], q = c[k] * r[i]; h[i] = p + q; }
    }
    hvec<V> out(n);
    for (size_t i = 0; i < n; i++) { const V p = V(1) * h[i]; out[i] = p + x[i]; }
    return out;
}

// ---- the reference's cases (testing/jacobi.cu, testing/polynomial.cu), for any matrix type ----
template <typename Matrix> void TestJacobiRelaxation()
{
    typedef typename Matrix::value_type V;
    typedef typename Matrix::memory_space Space;
    Matrix A(dense<V>(5, {1, 1, 2, 0, 0, 3, 2, 0, 0, 5, 0, 0, 0.5, 0, 0, 0, 6, 7, 4, 0, 0, 8, 0, 0, 8}));
    cusp::array1d<V, Space> b(5, V(5)), x(5, V(-1));
    cusp::relaxation::jacobi<V, Space> relax(A);
    relax(A, b, x);
    const V want[5] = {8, 6.5, 10, 4.5, 1.625}; // every step is exact in binary: equality, not a tolerance
    hvec<V> got(x);
    for (int i = 0; i < 5; i++) ASSERT_EQUAL(got[i], want[i]);
}
template <typename Matrix> void TestJacobiRelaxationWithWeighting()
{
    typedef typename Matrix::value_type V;
    typedef typename Matrix::memory_space Space;
    Matrix A(dense<V>(2, {2, 1, 1, 3}));
    { // the constructor's omega
        cusp::array1d<V, Space> b(2, V(5)), x(2, V(-1));
        cusp::relaxation::jacobi<V, Space> relax(A, V(0.5));
        relax(A, b, x);
        hvec<V> got(x);
        ASSERT_EQUAL(got[0], V(1)); // -1 + 0.5 * 8 / 2 and -1 + 0.5 * 9 / 3: exact
        ASSERT_EQUAL(got[1], V(0.5));
    }
    { // overridden
        cusp::array1d<V, Space> b(2, V(5)), x(2, V(-1));
        cusp::relaxation::jacobi<V, Space> relax(A, V(1));
        relax(A, b, x, V(0.5));
        hvec<V> got(x);
        ASSERT_EQUAL(got[0], V(1));
        ASSERT_EQUAL(got[1], V(0.5));
    }
}
// |got - want| <= 64 eps max|want|: both sides are sums of at most a dozen terms of magnitude <= max|want| evaluated in a different order
template <typename V> void assert_close(const hvec<V> &got, const hvec<V> &want)
{
    V big = 1;
    for (size_t i = 0; i < want.size(); i++) big = std::max(big, std::abs(want[i]));
    for (size_t i = 0; i < want.size(); i++) ASSERT_TRUE(std::abs(got[i] - want[i]) <= 64 * std::numeric_limits<V>::epsilon() * big);
}
template <typename Matrix> void TestPolynomialRelaxation()
{
    typedef typename Matrix::value_type V;
    typedef typename Matrix::memory_space Space;
    Matrix A(dense<V>(5, {2, -1, 0, 0, 0, -1, 2, -1, 0, 0, 0, -1, 2, -1, 0, 0, 0, -1, 2, -1, 0, 0, 0, -1, 2}));
    cusp::array1d<V, Space> b(5, V(0)), x0(5);
    for (int i = 0; i < 5; i++) x0[i] = V(i);
    cusp::array1d<V, Space> residual(5);
    cusp::multiply(A, x0, residual);
    cusp::blas::axpby(b, residual, residual, V(1), V(-1));
    { // degree 1: x0 + c r
        cusp::array1d<V, Space> x(x0), coef(1, V(-1.0 / 3.0)), expected(5);
        cusp::relaxation::polynomial<V, Space> relax(A, coef);
        ASSERT_EQUAL(relax.default_coefficients.size(), (size_t)0);
        cusp::blas::axpby(x0, residual, expected, V(1), V(-1.0 / 3.0));
        relax(A, b, x, coef);
        assert_close(hvec<V>(x), hvec<V>(expected));
    }
    { // three coefficients: x0 + c0 A^2 r + c1 A r + c2 r
        cusp::array1d<V, Space> coef(3);
        coef[0] = V(-0.14285714); coef[1] = V(1); coef[2] = V(-2);
        cusp::relaxation::polynomial<V, Space> relax(A, coef);
        ASSERT_EQUAL(relax.default_coefficients.size(), (size_t)2);
        ASSERT_EQUAL(relax.default_coefficients[0], -V(-0.14285714));
        ASSERT_EQUAL(relax.default_coefficients[1], V(-1));
        cusp::array1d<V, Space> Ar(5), A2r(5), expected(5), x(x0);
        cusp::multiply(A, residual, Ar);
        cusp::multiply(A, Ar, A2r);
        cusp::blas::axpby(x0, A2r, expected, V(1), V(-0.14285714));
        cusp::blas::axpby(expected, Ar, expected, V(1), V(1));
        cusp::blas::axpby(expected, residual, expected, V(1), V(-2));
        relax(A, b, x, coef);
        assert_close(hvec<V>(x), hvec<V>(expected));
    }
}

// ---- any format, any space, against the naive restatement on the host CSR matrix: bit for bit ----
template <typename Matrix> void check_against_naive(const hcsr<typename Matrix::value_type> &H, uint64_t salt)
{
    typedef typename Matrix::value_type V;
    typedef typename Matrix::memory_space Space;
    const size_t n = H.num_rows;
    Matrix A(H);
    const hvec<V> hb = seeded_vector<V>(n, salt + 1), hx = seeded_vector<V>(n, salt + 2);
    const cusp::array1d<V, Space> b(hb);
    { // Jacobi: default omega and an overriding one whose products round; x's storage stays where it is
        cusp::relaxation::jacobi<V, Space> relax(A, V(2.0 / 3.0));
        ASSERT_TRUE(bits_equal(hvec<V>(relax.diagonal), naive_diagonal(H)));
        cusp::array1d<V, Space> x(hx);
        const V *where = x.data();
        relax(A, b, x);
        ASSERT_TRUE(x.data() == where);
        const hvec<V> once = naive_jacobi(H, hb, hx, V(2.0 / 3.0));
        ASSERT_TRUE(bits_equal(hvec<V>(x), once));
        relax(A, b, x, V(0.7));
        ASSERT_TRUE(x.data() == where);
        ASSERT_TRUE(bits_equal(hvec<V>(x), naive_jacobi(H, hb, once, V(0.7))));
    }
    { // polynomial: two successive calls on ONE object (its buffers carry no stale state), then the zero-norm shortcut
        const std::vector<V> given = {V(0.3), V(-1.1), V(0.7), V(5)}, kept = {V(-0.3), V(1.1), V(-0.7)};
        cusp::relaxation::polynomial<V, Space> relax(A, hvec<V>(given));
        hvec<V> h(n, V(0));
        cusp::array1d<V, Space> x(hx);
        relax(A, b, x);
        const hvec<V> first = naive_polynomial(H, hb, hx, kept, h);
        ASSERT_TRUE(bits_equal(hvec<V>(x), first));
        ASSERT_TRUE(bits_equal(hvec<V>(relax.h), h));
        relax(A, b, x);
        const hvec<V> second = naive_polynomial(H, hb, first, kept, h);
        ASSERT_TRUE(bits_equal(hvec<V>(x), second));
        const std::vector<V> two = {V(-1.0 / 3.0), V(0.9)}; // explicit coefficients: used as given
        relax(A, b, x, hvec<V>(two));
        const hvec<V> third = naive_polynomial(H, hb, second, two, h);
        ASSERT_TRUE(bits_equal(hvec<V>(x), third));
        cusp::array1d<V, Space> zero(n, V(0));
        relax(A, b, zero);
        ASSERT_TRUE(bits_equal(hvec<V>(zero), naive_polynomial(H, hb, hvec<V>(n, V(0)), kept, h)));
        ASSERT_TRUE(bits_equal(hvec<V>(relax.residual), hb));
    }
}

template <typename Matrix> void TestAgainstNaive()
{
    typedef typename Matrix::value_type V;
    check_against_naive<Matrix>(seeded_stencil<V>(23, 17, 5), 11);  // 391 rows, none exact: not a multiple of any tile of the multiply or of the elementwise kernels
    check_against_naive<Matrix>(seeded_stencil<V>(1, 1, 9), 13);    // 1 x 1
}

} // namespace relax_check
