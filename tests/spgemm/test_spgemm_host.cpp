// cusp::multiply(A, B, C) with three sparse host_memory matrices: csr x csr -> csr and coo x coo -> coo, the six-argument form, policies,
// aliasing and shape errors, against the naive chain of spgemm_check.h with its zeros dropped.  Built and run by tests/test_spgemm_host.py.
//   test_spgemm_host                          runs the tests
//   test_spgemm_host --product f64|f32 A.mtx B.mtx   prints C = A B (rows sorted by column first) as text with the values' bit patterns
#include <cinttypes>
#include <cstdio>
#include "spgemm_check.h"

using namespace spgemm_check;

template <typename V> void TestHostCsrProduct()
{
    for (uint64_t salt : {1, 2, 3}) {
        host_csr<V> A = irregular<V>(40 + salt, 30, 9, salt), B = irregular<V>(30, 50 + salt, 7, 100 + salt), C;
        cusp::multiply(A, B, C);
        ASSERT_TRUE(csr_bits_equal(C, naive(A, B, false)));
        ASSERT_TRUE(rows_strictly_ascending(C));
        ASSERT_EQUAL(C.num_rows, A.num_rows);
        ASSERT_EQUAL(C.num_cols, B.num_cols);
    }
    host_csr<V> E(5, 4, 0), B = irregular<V>(4, 6, 3, 7), C; // no entries at all
    for (size_t i = 0; i <= 5; i++) E.row_offsets[i] = 0;
    cusp::multiply(E, B, C);
    ASSERT_EQUAL(C.num_entries, (size_t)0);
    ASSERT_EQUAL(C.num_rows, (size_t)5);
    ASSERT_EQUAL(C.num_cols, (size_t)6);
}
void TestHostCsrProductF64() { TestHostCsrProduct<double>(); }
void TestHostCsrProductF32() { TestHostCsrProduct<float>(); }
DECLARE_UNITTEST(TestHostCsrProductF64);
DECLARE_UNITTEST(TestHostCsrProductF32);

void TestHostPoissonSquaredKnownAnswer()
{
    // (A A)(i, i) of the 5-point Laplacian = 16 + its number of neighbours; small integers: exact
    host_csr<double> A, C;
    cusp::gallery::poisson5pt(A, 6, 5);
    cusp::multiply(A, A, C);
    ASSERT_TRUE(csr_bits_equal(C, naive(A, A, false)));
    for (size_t i = 0; i < C.num_rows; i++)
        for (int q = C.row_offsets[i]; q < C.row_offsets[i + 1]; q++)
            if (C.column_indices[q] == (int)i) ASSERT_EQUAL(C.values[q], 16.0 + (A.row_offsets[i + 1] - A.row_offsets[i] - 1));
}
DECLARE_UNITTEST(TestHostPoissonSquaredKnownAnswer);

void TestHostDropsZerosSortsRowsStartsAtPlusZero()
{
    // row 0: an exact cancellation in column 0 (dropped) and 5 in column 1; touched in the order 1, 0.  row 1: a lone product of -0.0 (dropped: it
    // compares equal to zero).  row 2: column 0 is the chain 2^53 + 1 + 1 + 2^53 + 1 over a duplicate column of A and of B = 2^54 (every 1 is lost);
    // summed in reverse the ones would survive
    const double big = 9007199254740992.0;
    host_csr<double> A = from_rows<double>(3, 3, {{{0, 1.0}, {1, 1.0}}, {{0, -0.0}}, {{2, 1.0}, {0, 1.0}, {2, 1.0}}});
    host_csr<double> B = from_rows<double>(3, 2, {{{1, 5.0}, {0, 1.0}}, {{0, -1.0}}, {{0, big}, {0, 1.0}}});
    host_csr<double> C;
    cusp::multiply(A, B, C);
    ASSERT_TRUE(csr_bits_equal(C, naive(A, B, false)));
    ASSERT_EQUAL(C.row_offsets[1], 1);
    ASSERT_EQUAL(C.column_indices[0], 1);
    ASSERT_EQUAL(C.values[0], 5.0);
    ASSERT_EQUAL(C.row_offsets[2], 1);
    ASSERT_EQUAL(C.row_offsets[3], 3);
    ASSERT_EQUAL(C.values[1], 2 * big);
}
DECLARE_UNITTEST(TestHostDropsZerosSortsRowsStartsAtPlusZero);

template <typename V> void TestHostCooProduct()
{
    host_csr<V> A = irregular<V>(33, 21, 8, 11), B = irregular<V>(21, 27, 6, 12), C;
    cusp::multiply(A, B, C);
    cusp::coo_matrix<int, V, cusp::host_memory> cA, cB, cC;
    cusp::convert(A, cA);
    cusp::convert(B, cB);
    cusp::multiply(cA, cB, cC);
    host_csr<V> back;
    cusp::convert(cC, back);
    ASSERT_TRUE(csr_bits_equal(back, C));
    ASSERT_TRUE(cC.is_sorted_by_row_and_column());
}
void TestHostCooProductF64() { TestHostCooProduct<double>(); }
void TestHostCooProductF32() { TestHostCooProduct<float>(); }
DECLARE_UNITTEST(TestHostCooProductF64);
DECLARE_UNITTEST(TestHostCooProductF32);

struct maxf { double operator()(double a, double b) const { return a > b ? a : b; } };

void TestHostSixArgumentForm()
{
    host_csr<double> A = irregular<double>(20, 15, 6, 21), B = irregular<double>(15, 18, 6, 22), C, D;
    cusp::multiply(A, B, C);
    cusp::multiply(A, B, D, cusp::constant_functor<double>(0.0), cusp::multiplies<double>(), cusp::plus<double>());
    ASSERT_TRUE(csr_bits_equal(C, D));
    // any functors on the host: reduce = max over the entry's products and 0 (the chain starts at 0), combine = plus
    cusp::multiply(A, B, D, cusp::constant_functor<double>(0.0), cusp::plus<double>(), maxf());
    for (size_t i = 0; i < D.num_rows; i++)
        for (int q = D.row_offsets[i]; q < D.row_offsets[i + 1]; q++) {
            double want = 0.0;
            for (int jj = A.row_offsets[i]; jj < A.row_offsets[i + 1]; jj++)
                for (int kk = B.row_offsets[A.column_indices[jj]]; kk < B.row_offsets[A.column_indices[jj] + 1]; kk++)
                    if (B.column_indices[kk] == D.column_indices[q]) want = maxf()(want, A.values[jj] + B.values[kk]);
            ASSERT_EQUAL(D.values[q], want);
            ASSERT_TRUE(want != 0.0);
        }
    ASSERT_TRUE(D.num_entries > 0);
}
DECLARE_UNITTEST(TestHostSixArgumentForm);

void TestHostPoliciesAliasingAndShapes()
{
    host_csr<double> A = irregular<double>(25, 25, 6, 31), C, D, E;
    cusp::multiply(A, A, C);
    cusp::multiply(cusp::omp::par, A, A, D);
    ASSERT_TRUE(csr_bits_equal(C, D));
    cusp::multiply(cusp::hip::par, A, A, E);
    ASSERT_TRUE(csr_bits_equal(C, E));
    host_csr<double> S = A;
    cusp::multiply(S, S, S); // C may be an operand
    ASSERT_TRUE(csr_bits_equal(C, S));
    host_csr<double> R = irregular<double>(24, 7, 3, 32);
    ASSERT_THROWS(cusp::multiply(A, R, C), cusp::invalid_input_exception);
}
DECLARE_UNITTEST(TestHostPoliciesAliasingAndShapes);

template <typename V> int print_product(const char *fa, const char *fb)
{
    cusp::coo_matrix<int, V, cusp::host_memory> a, b;
    cusp::io::read_matrix_market_file(a, fa);
    cusp::io::read_matrix_market_file(b, fb);
    a.sort_by_row_and_column();
    b.sort_by_row_and_column();
    host_csr<V> A, B, C;
    cusp::convert(a, A);
    cusp::convert(b, B);
    cusp::multiply(A, B, C);
    std::printf("%zu %zu %zu\n", C.num_rows, C.num_cols, C.num_entries);
    for (size_t i = 0; i <= C.num_rows; i++) std::printf("%d ", (int)C.row_offsets[i]);
    std::printf("\n");
    for (size_t q = 0; q < C.num_entries; q++) {
        const V v = C.values[q];
        uint64_t bits = 0;
        std::memcpy(&bits, &v, sizeof(V));
        std::printf("%d %" PRIx64 "\n", (int)C.column_indices[q], bits);
    }
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 5 && std::string(argv[1]) == "--product")
        return std::string(argv[2]) == "f32" ? print_product<float>(argv[3], argv[4]) : print_product<double>(argv[3], argv[4]);
    return unittest::run_all(argc, argv);
}
