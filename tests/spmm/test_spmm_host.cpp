// cusp::multiply(A, X, Y) with array2d X and Y on host_memory CSR matrices (and views): the sequential loop, its OpenMP
// form, functor variants and shape errors, against a naive storage-order loop.  Built and run by tests/test_spmm_host.py;
// argv[1]: a MatrixMarket file of the irregular golden fixture.
#include <cstring>
#include "spmm_check.h"

using namespace spmm_check;
static std::string g_irregular;

// the matrices of the reference's TestSparseMatrixDenseMatrixMultiply (testing/multiply.cu:289-376): dense -> CSR,
// left x right for every compatible pair, against the dense product (small integers: exact)
static cusp::array2d<double, cusp::host_memory> dense(size_t r, size_t c, std::vector<double> v)
{
    cusp::array2d<double, cusp::host_memory> a(r, c);
    for (size_t i = 0; i < r; i++)
        for (size_t j = 0; j < c; j++) a(i, j) = v[i * c + j];
    return a;
}
static cusp::csr_matrix<int, double, cusp::host_memory> to_csr(const cusp::array2d<double, cusp::host_memory> &d)
{
    size_t nnz = 0;
    for (size_t i = 0; i < d.num_rows; i++)
        for (size_t j = 0; j < d.num_cols; j++) nnz += d(i, j) != 0.0;
    cusp::csr_matrix<int, double, cusp::host_memory> A(d.num_rows, d.num_cols, nnz);
    size_t n = 0;
    A.row_offsets[0] = 0;
    for (size_t i = 0; i < d.num_rows; i++) {
        for (size_t j = 0; j < d.num_cols; j++)
            if (d(i, j) != 0.0) { A.column_indices[n] = (int)j; A.values[n] = d(i, j); n++; }
        A.row_offsets[i + 1] = (int)n;
    }
    return A;
}

void TestSparseMatrixDenseMatrixMultiplyKnownAnswer()
{
    std::vector<cusp::array2d<double, cusp::host_memory>> m;
    m.push_back(dense(3, 2, {1, 2, 3, 0, 5, 6}));
    m.push_back(dense(2, 4, {0, 2, 3, 4, 5, 0, 0, 8}));
    m.push_back(dense(2, 2, {0, 0, 3, 5}));
    m.push_back(dense(2, 1, {2, 3}));
    m.push_back(dense(2, 2, {0, 0, 0, 0}));
    m.push_back(dense(2, 3, {0, 1.5, 3, 0.5, 0, 0}));
    int pairs = 0;
    for (auto &l : m)
        for (auto &r : m) {
            if (l.num_cols != r.num_rows) continue;
            cusp::csr_matrix<int, double, cusp::host_memory> A = to_csr(l);
            cusp::array2d<double, cusp::host_memory> Y(l.num_rows, r.num_cols, -1.0), W(l.num_rows, r.num_cols, 0.0);
            for (size_t i = 0; i < l.num_rows; i++)
                for (size_t c = 0; c < r.num_cols; c++)
                    for (size_t j = 0; j < l.num_cols; j++) W(i, c) += l(i, j) * r(j, c);
            cusp::multiply(A, r, Y);
            for (size_t i = 0; i < l.num_rows; i++)
                for (size_t c = 0; c < r.num_cols; c++) ASSERT_EQUAL(Y(i, c), W(i, c));
            pairs++;
        }
    ASSERT_TRUE(pairs >= 10);
    // the exact answer of A x B from the reference's matrices
    cusp::array2d<double, cusp::host_memory> Y(3, 4);
    cusp::multiply(to_csr(m[0]), m[1], Y);
    const double want[12] = {10, 2, 3, 20, 0, 6, 9, 12, 30, 10, 15, 68};
    for (size_t i = 0; i < 3; i++)
        for (size_t c = 0; c < 4; c++) ASSERT_EQUAL(Y(i, c), want[i * 4 + c]);
}
DECLARE_UNITTEST(TestSparseMatrixDenseMatrixMultiplyKnownAnswer);

// every layout combination of X and Y, padded pitches, accumulate, on one matrix
template <typename V, typename M> void check_layouts(const M &A, size_t k, uint64_t salt)
{
    typedef cusp::array2d<V, cusp::host_memory, cusp::row_major> R;
    typedef cusp::array2d<V, cusp::host_memory, cusp::column_major> C;
    R X(A.num_cols, k), Y0(A.num_rows, k), W(A.num_rows, k);
    fill(X, salt);
    fill(Y0, salt + 99);
    W = Y0;
    naive(A, X, W, false);
    { R Y = Y0; cusp::multiply(A, X, Y); ASSERT_TRUE(bits_equal(Y, W)); }
    { C Xc(X), Yc(Y0); cusp::multiply(A, Xc, Yc); ASSERT_TRUE(bits_equal(Yc, W)); }
    { C Xc(X); R Y = Y0; cusp::multiply(A, Xc, Y); ASSERT_TRUE(bits_equal(Y, W)); }
    { C Yc(Y0); cusp::multiply(A, X, Yc); ASSERT_TRUE(bits_equal(Yc, W)); }
    { // padded pitches
        R Xp(A.num_cols, k, V(0), k + 3), Yp(A.num_rows, k, V(7), k + 5);
        C Xq(A.num_cols, k, V(0), A.num_cols + 2);
        for (size_t i = 0; i < A.num_cols; i++)
            for (size_t c = 0; c < k; c++) Xp(i, c) = Xq(i, c) = X(i, c);
        cusp::multiply(A, Xp, Yp);
        ASSERT_TRUE(bits_equal(Yp, W));
        C Yq(A.num_rows, k, V(7), A.num_rows + 1);
        cusp::multiply(A, Xq, Yq);
        ASSERT_TRUE(bits_equal(Yq, W));
    }
    // Y = Y + A X: identity_function
    R Wa = Y0;
    naive(A, X, Wa, true);
    { R Y = Y0; cusp::multiply(A, X, Y, cusp::identity_function<V>(), cusp::multiplies<V>(), cusp::plus<V>()); ASSERT_TRUE(bits_equal(Y, Wa)); }
    // OpenMP: same bits
    { R Y = Y0; cusp::multiply(cusp::omp::par, A, X, Y); ASSERT_TRUE(bits_equal(Y, W)); }
    { C Y(Y0); cusp::multiply(cusp::omp::par, A, X, Y, cusp::identity_function<V>(), cusp::multiplies<V>(), cusp::plus<V>()); ASSERT_TRUE(bits_equal(Y, Wa)); }
    // the library's execution policy on host containers: ignored
    { R Y = Y0; cusp::multiply(cusp::hip::par, A, X, Y); ASSERT_TRUE(bits_equal(Y, W)); }
    // a view of the matrix
    { R Y = Y0; auto Av = cusp::make_csr_matrix_view(A); cusp::multiply(Av, X, Y); ASSERT_TRUE(bits_equal(Y, W)); }
}

template <typename V> void TestPoissonLayouts()
{
    cusp::csr_matrix<int, V, cusp::host_memory> A;
    cusp::gallery::poisson5pt(A, 30, 20);
    for (size_t k : {1, 2, 3, 8, 17}) check_layouts<V>(A, k, 11 + k);
}
void TestPoissonLayoutsF64() { TestPoissonLayouts<double>(); }
void TestPoissonLayoutsF32() { TestPoissonLayouts<float>(); }
DECLARE_UNITTEST(TestPoissonLayoutsF64);
DECLARE_UNITTEST(TestPoissonLayoutsF32);

template <typename V> void TestIrregularLayouts()
{
    check_layouts<V>(irregular<V>(300, 211, 5), 5, 3);
    if (!g_irregular.empty()) { // the golden irregular fixture (1500 x 1237)
        cusp::csr_matrix<int, V, cusp::host_memory> A;
        cusp::io::read_matrix_market_file(A, g_irregular);
        ASSERT_EQUAL(A.num_rows, (size_t)1500);
        for (size_t k : {2, 7}) check_layouts<V>(A, k, 40 + k);
    }
}
void TestIrregularLayoutsF64() { TestIrregularLayouts<double>(); }
void TestIrregularLayoutsF32() { TestIrregularLayouts<float>(); }
DECLARE_UNITTEST(TestIrregularLayoutsF64);
DECLARE_UNITTEST(TestIrregularLayoutsF32);

void TestGenericFunctorsOnHost()
{
    // host loops stay generic: max-plus on a small matrix
    cusp::csr_matrix<int, double, cusp::host_memory> A;
    cusp::gallery::poisson5pt(A, 4, 3);
    cusp::array2d<double, cusp::host_memory> X(12, 2), Y(12, 2, 0.0);
    fill(X, 1);
    struct maxf { double operator()(double a, double b) const { return a > b ? a : b; } };
    cusp::multiply(A, X, Y, cusp::constant_functor<double>(-1e300), cusp::plus<double>(), maxf());
    for (size_t i = 0; i < 12; i++)
        for (size_t c = 0; c < 2; c++) {
            double m = -1e300;
            for (int jj = A.row_offsets[i]; jj < A.row_offsets[i + 1]; jj++) m = std::max(m, A.values[jj] + X(A.column_indices[jj], c));
            ASSERT_EQUAL(Y(i, c), m);
        }
}
DECLARE_UNITTEST(TestGenericFunctorsOnHost);

void TestShapeMismatchThrows()
{
    cusp::csr_matrix<int, double, cusp::host_memory> A;
    cusp::gallery::poisson5pt(A, 4, 3); // 12 x 12
    cusp::array2d<double, cusp::host_memory> X(12, 3), Y(12, 3), Xbad(11, 3), Ybad(13, 3), Ywide(12, 4);
    ASSERT_THROWS(cusp::multiply(A, Xbad, Y), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::multiply(A, X, Ybad), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::multiply(A, X, Ywide), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::multiply(cusp::omp::par, A, X, Ywide), cusp::invalid_input_exception);
}
DECLARE_UNITTEST(TestShapeMismatchThrows);

void TestEmptyShapes()
{
    cusp::csr_matrix<int, double, cusp::host_memory> A(5, 4, 0); // nnz = 0
    for (size_t i = 0; i <= 5; i++) A.row_offsets[i] = 0;
    cusp::array2d<double, cusp::host_memory> X(4, 3, 1.0), Y(5, 3, 9.0);
    cusp::multiply(A, X, Y, cusp::identity_function<double>(), cusp::multiplies<double>(), cusp::plus<double>());
    for (size_t i = 0; i < 5; i++) ASSERT_EQUAL(Y(i, 2), 9.0);
    cusp::multiply(A, X, Y);
    for (size_t i = 0; i < 5; i++) ASSERT_EQUAL(Y(i, 0), 0.0);
    cusp::array2d<double, cusp::host_memory> X0(4, 0), Y0(5, 0);
    cusp::multiply(A, X0, Y0);
}
DECLARE_UNITTEST(TestEmptyShapes);

int main(int argc, char **argv)
{
    if (argc > 1) g_irregular = argv[1];
    return unittest::run_all(1, argv);
}
