// Shared by the cusp::eigen test programs (TEST_SPACE / TEST_SPACE_NAME are defined by the including program): the matrices and the
// criterion of tests/test_eigen_refs.py through the real headers in TEST_SPACE -- the four estimators on all five formats in float and
// double against the exact spectral radii, relative error < 0.1 (the reference's own criterion, testing/spectral_radius.cu; the margin
// over any start vector is threefold, see tests/test_eigen_refs.py), the Gershgorin bound against exact integers, the shape of the
// Hessenberg matrices (a 2 x 2 diagonal matrix gives a 2 x 2 block: the completed column is kept on breakdown), cusp::random_array in
// both memory spaces, operators without a storage format, and cusp::relaxation::make_chebyshev_polynomial.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include <cusp/array2d.h>
#include <cusp/coo_matrix.h>
#include <cusp/csr_matrix.h>
#include <cusp/dia_matrix.h>
#include <cusp/eigen/arnoldi.h>
#include <cusp/eigen/spectral_radius.h>
#include <cusp/ell_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/hyb_matrix.h>
#include <cusp/relaxation/chebyshev.h>

#include "unittest.h"

namespace eigen_check {

const double kPi = 3.14159265358979323846;
const double kTol = 0.1;
template <typename V> using hcsr = cusp::csr_matrix<int, V, cusp::host_memory>;
template <typename V> using hvec = cusp::array1d<V, cusp::host_memory>;

struct test_case { const char *name; size_t m, n; double rho, rho_dinv; }; // m == 0: diag(-5, 2)
inline double poisson_rho(size_t m, size_t n) { return 4 + 2 * std::cos(kPi / (m + 1)) + 2 * std::cos(kPi / (n + 1)); }
inline std::vector<test_case> cases()
{
    return {{"diag(-5,2)", 0, 0, 5.0, 1.0},
            {"poisson2x2", 2, 2, 6.0, 1.5},
            {"poisson37x41", 37, 41, poisson_rho(37, 41), poisson_rho(37, 41) / 4},
            {"poisson64x3", 64, 3, poisson_rho(64, 3), poisson_rho(64, 3) / 4},
            {"poisson130x9", 130, 9, poisson_rho(130, 9), poisson_rho(130, 9) / 4}};
}
template <typename V> hcsr<V> host_matrix(const test_case &c)
{
    hcsr<V> A;
    if (c.m) { cusp::gallery::poisson5pt(A, c.m, c.n); return A; }
    cusp::array2d<V, cusp::host_memory> D(2, 2, V(0));
    D(0, 0) = V(-5);
    D(1, 1) = V(2);
    return hcsr<V>(D);
}
inline void near(double got, double want, const char *what, const char *name)
{
    if (!(std::abs(got - want) / want < kTol)) {
        char msg[256];
        std::snprintf(msg, sizeof msg, "%s on %s in %s: %.9g, exact %.9g", what, name, TEST_SPACE_NAME, got, want);
        throw unittest::failure(msg);
    }
}

// every estimator on one format x value type
template <typename Matrix> void TestSpectralRadiusEstimators()
{
    typedef typename Matrix::value_type V;
    ASSERT_TRUE(std::abs(poisson_rho(37, 41) - 7.987577) < 1e-6 && std::abs(poisson_rho(64, 3) - 7.411878) < 1e-6 && std::abs(poisson_rho(130, 9) - 7.901538) < 1e-6);
    for (const test_case &c : cases()) {
        const Matrix A(host_matrix<V>(c));
        near(cusp::eigen::estimate_spectral_radius(A, 40), c.rho, "estimate_spectral_radius(A, 40)", c.name);
        near(cusp::eigen::ritz_spectral_radius(A), c.rho, "ritz_spectral_radius(A)", c.name);
        near(cusp::eigen::ritz_spectral_radius(A, 10, true), c.rho, "ritz_spectral_radius(A, 10, true)", c.name);
        near(cusp::eigen::ritz_spectral_radius(A, 8, true), c.rho, "ritz_spectral_radius(A, 8, true)", c.name);
        near(cusp::eigen::estimate_rho_Dinv_A(A), c.rho_dinv, "estimate_rho_Dinv_A(A)", c.name);
    }
}

// the Gershgorin bound: exact integers
template <typename Matrix> void TestDisksSpectralRadius()
{
    typedef typename Matrix::value_type V;
    const test_case list[4] = {{"diag(-5,2)", 0, 0, 5, 0}, {"poisson2x2", 2, 2, 6, 0}, {"poisson4x4", 4, 4, 8, 0}, {"poisson37x41", 37, 41, 8, 0}};
    for (const test_case &c : list) {
        const Matrix A(host_matrix<V>(c));
        ASSERT_EQUAL(cusp::eigen::disks_spectral_radius(A), c.rho);
        ASSERT_EQUAL(cusp::eigen::detail::disks_spectral_radius(A, std::false_type()), c.rho); // the generic sequence: one host copy in CSR form
    }
    const Matrix E(hcsr<V>(0, 0, 0));
    ASSERT_EQUAL(cusp::eigen::disks_spectral_radius(E), 0.0);
}

template <typename V, typename Space> void hessenberg_shapes()
{
    typedef cusp::csr_matrix<int, V, Space> Csr;
    // a 2 x 2 diagonal matrix: breakdown at step 1, the completed column stays
    const Csr D(host_matrix<V>(cases()[0]));
    cusp::array2d<V, cusp::host_memory> H;
    cusp::eigen::arnoldi(D, H, 10);
    ASSERT_EQUAL(H.num_rows, (size_t)2);
    ASSERT_EQUAL(H.num_cols, (size_t)2);
    ASSERT_TRUE(std::abs((double)H(0, 0) + (double)H(1, 1) + 3.0) < 1e-4);                                          // the trace of diag(-5, 2)
    ASSERT_TRUE(std::abs((double)H(0, 0) * (double)H(1, 1) - (double)H(0, 1) * (double)H(1, 0) + 10.0) < 1e-3);      // and its determinant
    cusp::eigen::detail::lanczos_estimate(D, H, 10);
    ASSERT_EQUAL(H.num_rows, (size_t)2);
    ASSERT_TRUE(std::abs((double)H(0, 0) + (double)H(1, 1) + 3.0) < 1e-4);
    ASSERT_EQUAL(H(0, 1), H(1, 0));
    // Poisson 37 x 41: no breakdown, k x k, upper Hessenberg with a positive subdiagonal; Lanczos: the same tridiagonal part
    const Csr P(host_matrix<V>(cases()[2]));
    cusp::array2d<V, cusp::host_memory> T;
    cusp::eigen::arnoldi(P, H, 10);
    cusp::eigen::detail::lanczos_estimate(P, T, 10);
    ASSERT_EQUAL(H.num_rows, (size_t)10);
    ASSERT_EQUAL(H.num_cols, (size_t)10);
    ASSERT_EQUAL(T.num_rows, (size_t)10);
    for (size_t i = 0; i < 10; i++)
        for (size_t j = 0; j < 10; j++) {
            if (i > j + 1) { ASSERT_EQUAL(H(i, j), V(0)); }
            if (i > j + 1 || j > i + 1) { ASSERT_EQUAL(T(i, j), V(0)); }
            if (i == j + 1) { ASSERT_TRUE(H(i, j) > V(0)); ASSERT_TRUE(T(i, j) > V(0)); ASSERT_EQUAL(T(i, j), T(j, i)); }
        }
    ASSERT_EQUAL(H(0, 0), T(0, 0)); // step 0 is the same operations in both loops: the same bits
    ASSERT_EQUAL(H(1, 0), T(1, 0));
    // fewer rows than steps: min(N, k) steps
    cusp::eigen::arnoldi(Csr(host_matrix<V>(cases()[1])), H, 10);
    ASSERT_TRUE(H.num_rows <= (size_t)4 && H.num_rows >= (size_t)2);
    cusp::eigen::arnoldi(P, H, 0);
    ASSERT_EQUAL(H.num_rows, (size_t)0);
}
template <typename Space> void TestHessenbergShapes()
{
    hessenberg_shapes<float, Space>();
    hessenberg_shapes<double, Space>();
}

template <typename V, typename Space> void random_arrays()
{
    const size_t n = 1025;
    hvec<V> h, h7;
    cusp::copy(cusp::random_array<V>(n), h);
    cusp::copy(cusp::random_array<V>(n, 7), h7);
    ASSERT_EQUAL(h.size(), n);
    bool all_equal = true, differ = false;
    for (size_t i = 0; i < n; i++) {
        ASSERT_TRUE(h[i] >= V(0) && h[i] < V(1));
        if (h[i] != h[0]) all_equal = false;
        if (h[i] != h7[i]) differ = true;
        ASSERT_EQUAL(h[i], cusp::random_array<V>(n)[i]);
    }
    ASSERT_TRUE(!all_equal && differ);
    // the same bits wherever the copy lands
    cusp::array1d<V, Space> d;
    cusp::copy(cusp::random_array<V>(n, 7), d);
    const hvec<V> back(d);
    ASSERT_TRUE(std::memcmp(back.data(), h7.data(), n * sizeof(V)) == 0);
    cusp::array1d<V, Space> none(3, V(1));
    cusp::copy(cusp::random_array<V>(0), none);
    ASSERT_EQUAL(none.size(), (size_t)0);
}
template <typename Space> void TestRandomArray()
{
    random_arrays<float, Space>();
    random_arrays<double, Space>();
    ASSERT_EQUAL(cmi_random_hash(0, 0), (uint64_t)0xE220A8397B1DCDAFull); // splitmix64's first output for seed 0
}

// an operator without a storage format: the identity breaks down at step 0 -- the 1 x 1 block [1] (the reference's rule: 0 x 0)
template <typename Space> void TestLinearOperators()
{
    const cusp::identity_operator<double, Space> I(50, 50);
    ASSERT_TRUE(std::abs(cusp::eigen::estimate_spectral_radius(I, 5) - 1.0) < 1e-12);
    ASSERT_TRUE(std::abs(cusp::eigen::ritz_spectral_radius(I, 8) - 1.0) < 1e-12);
    ASSERT_TRUE(std::abs(cusp::eigen::ritz_spectral_radius(I, 8, true) - 1.0) < 1e-12);
    const cusp::csr_matrix<int, float, Space> P(host_matrix<float>(cases()[3]));
    const cusp::eigen::detail::Dinv_A<cusp::csr_matrix<int, float, Space>> DA(P);
    near(cusp::eigen::estimate_spectral_radius(DA, 40), cases()[3].rho_dinv, "estimate_spectral_radius(Dinv_A, 40)", "poisson64x3");
}

template <typename V, typename Space> void chebyshev_factory()
{
    typedef cusp::csr_matrix<int, V, Space> Csr;
    hcsr<V> HP;
    cusp::gallery::poisson5pt(HP, 21, 17);
    const Csr A(HP);
    cusp::relaxation::polynomial<V, Space> M = cusp::relaxation::make_chebyshev_polynomial<V, Space>(A);
    hvec<V> want;
    cusp::relaxation::detail::chebyshev_polynomial_coefficients(static_cast<V>(cusp::eigen::ritz_spectral_radius(A, 8, true)), want);
    ASSERT_EQUAL(want.size(), (size_t)4);
    ASSERT_EQUAL(M.default_coefficients.size(), (size_t)3);
    for (size_t i = 0; i < 3; i++) {
        const V a = M.default_coefficients[i], b = -want[i];
        ASSERT_TRUE(std::memcmp(&a, &b, sizeof(V)) == 0);
    }
    // one relax step with them lowers the residual of a Poisson system
    const size_t N = A.num_rows;
    cusp::array1d<V, Space> b(N, V(1)), x(N, V(0)), r(N);
    M(A, b, x);
    cusp::multiply(A, x, r);
    cusp::blas::axpby(b, r, r, V(1), V(-1));
    ASSERT_TRUE(cusp::blas::nrm2(r) < V(0.9) * cusp::blas::nrm2(b));
    // from another format
    const cusp::ell_matrix<int, V, Space> E(HP);
    cusp::relaxation::polynomial<V, Space> ME = cusp::relaxation::make_chebyshev_polynomial<V, Space>(E);
    ASSERT_EQUAL(ME.default_coefficients.size(), (size_t)3);
}
template <typename Space> void TestChebyshevFactory()
{
    chebyshev_factory<float, Space>();
    chebyshev_factory<double, Space>();
}

} // namespace eigen_check
