// cusp::relaxation::jacobi and polynomial on host_memory: the cases of the reference's testing/jacobi.cu and
// testing/polynomial.cu on all five formats in float and double, the same classes against naive restatements bit for
// bit, the Chebyshev coefficients, and the argument errors.  Built and run by tests/test_relaxation_host.py (also under
// AddressSanitizer + UndefinedBehaviorSanitizer).
#define TEST_SPACE cusp::host_memory
#define TEST_SPACE_NAME "host_memory"
#include "relax_check.h"

using namespace relax_check;

DECLARE_SPARSE_MATRIX_UNITTEST(TestJacobiRelaxation);
DECLARE_SPARSE_MATRIX_UNITTEST(TestJacobiRelaxationWithWeighting);
DECLARE_SPARSE_MATRIX_UNITTEST(TestPolynomialRelaxation);
DECLARE_SPARSE_MATRIX_UNITTEST(TestAgainstNaive);

void TestChebyshevCoefficients()
{
    cusp::array1d<double, cusp::host_memory> coef;
    cusp::relaxation::detail::chebyshev_polynomial_coefficients(1.0, coef, 1.0, 2.0);
    const double want[4] = {-0.32323232, 1.45454545, -2.12121212, 1.0}; // the reference test's literals: 8 digits
    ASSERT_EQUAL(coef.size(), (size_t)4);
    for (int i = 0; i < 4; i++) ASSERT_TRUE(std::abs(coef[i] - want[i]) < 5e-9);
    cusp::array1d<float, cusp::host_memory> cf;
    cusp::relaxation::detail::chebyshev_polynomial_coefficients(2.0f, cf); // the default bounds, in float
    ASSERT_EQUAL(cf.size(), (size_t)4);
    ASSERT_EQUAL(cf[3], 1.0f);
}
DECLARE_UNITTEST(TestChebyshevCoefficients);

void TestDenseOperatorOnHost()
{
    // an array2d as the operator: the host sequence through cusp::multiply's dense loop
    cusp::array2d<double, cusp::host_memory> M = dense<double>(2, {2, 1, 1, 3});
    cusp::array1d<double, cusp::host_memory> b(2, 5.0), x(2, -1.0);
    cusp::relaxation::jacobi<double, cusp::host_memory> relax(M, 0.5);
    relax(M, b, x);
    ASSERT_EQUAL(x[0], 1.0);
    ASSERT_EQUAL(x[1], 0.5);
}
DECLARE_UNITTEST(TestDenseOperatorOnHost);

void TestArgumentErrors()
{
    cusp::csr_matrix<int, double, cusp::host_memory> A = seeded_stencil<double>(4, 3, 1);
    cusp::array1d<double, cusp::host_memory> b(12, 1.0), x(12, 1.0), shorter(11, 1.0), none;
    cusp::relaxation::jacobi<double, cusp::host_memory> J(A);
    ASSERT_THROWS(J(A, shorter, x), cusp::invalid_input_exception);
    ASSERT_THROWS(J(A, b, shorter), cusp::invalid_input_exception);
    cusp::relaxation::polynomial<double, cusp::host_memory> P(A, b);
    ASSERT_THROWS(P(A, shorter, x), cusp::invalid_input_exception);
    ASSERT_THROWS(P(A, b, x, none), cusp::invalid_input_exception);
    ASSERT_THROWS((cusp::relaxation::polynomial<double, cusp::host_memory>(A, none)), cusp::invalid_input_exception);
    // a zero on the diagonal: what IEEE division gives (inf here), as in the reference
    cusp::csr_matrix<int, double, cusp::host_memory> Z(2, 2, 1);
    Z.row_offsets[0] = 0; Z.row_offsets[1] = 1; Z.row_offsets[2] = 1;
    Z.column_indices[0] = 0; Z.values[0] = 2.0;
    cusp::array1d<double, cusp::host_memory> b2(2, 3.0), x2(2, 1.0);
    cusp::relaxation::jacobi<double, cusp::host_memory> JZ(Z);
    JZ(Z, b2, x2);
    ASSERT_EQUAL(x2[0], 1.5);
    ASSERT_TRUE(std::isinf(x2[1]) && x2[1] > 0);
}
DECLARE_UNITTEST(TestArgumentErrors);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }
