// The AINV preconditioners on host_memory (built by tests/test_ainv_host.py, plainly and under the address and undefined-behaviour sanitizers):
// the heap of a factor row, the reference's three tests in float, the pivot and shape exceptions, the five formats as input.
// "--dump f64|f32" prints the factors the Python side compares with tests/ainv_refs.py bit for bit.
#include "ainv_check.h"

#define TEST_SPACE cusp::host_memory
#define TEST_SPACE_NAME "host_memory"

using namespace ainv_check;
namespace precond = cusp::precond;

void TestAINVHeap() { heap_test(300); }
DECLARE_UNITTEST(TestAINVHeap);

// the tie rules, on values chosen to tie: the first child wins a tie in sift-down, an equal term replaces the minimum, a smaller one does not
void TestAINVHeapTies()
{
    precond::detail::ainv_matrix_row<int, double> row;
    row.insert(0, 1.0);
    row.insert(1, -2.0);
    row.insert(2, 2.0);
    ASSERT_EQUAL(row.min_abs_value(), 1.0);
    row.remove_min(); // the root goes: slot 2 (index 2) becomes the root and, tied with its only child (index 1), stays there
    ASSERT_EQUAL(row.min_abs_value(), 2.0);
    ASSERT_EQUAL(row.validate_backpointers(), true);
    row.replace_min_if_greater(7, 1.5); // strictly smaller than the minimum: refused
    ASSERT_EQUAL(row.has_entry_at_index(7), false);
    row.replace_min_if_greater(7, -2.0); // equal in magnitude: replaces it
    ASSERT_EQUAL(row.has_entry_at_index(7), true);
    ASSERT_EQUAL(row.has_entry_at_index(2), false);
    ASSERT_EQUAL(row.size(), (size_t)2);
    row.mult_by_scalar(-0.5);
    ASSERT_EQUAL(row.begin()->second.value, 1.0);
    const precond::detail::ainv_matrix_row<int, float> empty;
    ASSERT_EQUAL(empty.min_abs_value(), 0.0f);
}
DECLARE_UNITTEST(TestAINVHeapTies);

void TestAINVFactorization() { exact_factorisation_case<float, cusp::host_memory>(); }
DECLARE_UNITTEST(TestAINVFactorization);

void TestAINVSymmetry() { symmetry_case<float, cusp::host_memory>(); }
DECLARE_UNITTEST(TestAINVSymmetry);

void TestAINVConvergenceScaled() { convergence_cases<float, cusp::host_memory, precond::scaled_bridson_ainv>("scaled_bridson_ainv"); }
void TestAINVConvergenceBridson() { convergence_cases<float, cusp::host_memory, precond::bridson_ainv>("bridson_ainv"); }
DECLARE_UNITTEST(TestAINVConvergenceScaled);
DECLARE_UNITTEST(TestAINVConvergenceBridson);

// a zero pivot (row 1 of [[1, 1], [1, 1]]), a pivot that is not positive (-I), a matrix that is not square: cusp::invalid_input_exception naming the row
template <typename V> void TestAINVRefusals()
{
    host_csr<V> S(2, 2, 4);
    S.row_offsets[0] = 0; S.row_offsets[1] = 2; S.row_offsets[2] = 4;
    for (int e = 0; e < 4; e++) { S.column_indices[e] = e % 2; S.values[e] = 1; }
    ASSERT_THROWS((precond::bridson_ainv<V, cusp::host_memory>(S, 0)), cusp::invalid_input_exception);
    ASSERT_THROWS((precond::nonsym_bridson_ainv<V, cusp::host_memory>(S, 0)), cusp::invalid_input_exception);
    ASSERT_THROWS((precond::scaled_bridson_ainv<V, cusp::host_memory>(S, 0)), cusp::invalid_input_exception);
    try {
        precond::bridson_ainv<V, cusp::host_memory> M(S, 0);
    } catch (const cusp::invalid_input_exception &e) {
        ASSERT_TRUE(std::string(e.what()).find("row 1") != std::string::npos);
    }
    host_csr<V> N(2, 2, 2);
    N.row_offsets[0] = 0; N.row_offsets[1] = 1; N.row_offsets[2] = 2;
    for (int e = 0; e < 2; e++) { N.column_indices[e] = e; N.values[e] = -1; }
    ASSERT_THROWS((precond::scaled_bridson_ainv<V, cusp::host_memory>(N, 0)), cusp::invalid_input_exception);
    precond::bridson_ainv<V, cusp::host_memory> ok(N, 0); // a negative pivot is none of bridson_ainv's business
    ASSERT_EQUAL(ok.diagonals[0], V(-1));
    host_csr<V> R(2, 3, 0);
    R.row_offsets[0] = R.row_offsets[1] = R.row_offsets[2] = 0;
    ASSERT_THROWS((precond::bridson_ainv<V, cusp::host_memory>(R)), cusp::invalid_input_exception);
    ASSERT_THROWS((precond::scaled_bridson_ainv<V, cusp::host_memory>(R)), cusp::invalid_input_exception);
    ASSERT_THROWS((precond::nonsym_bridson_ainv<V, cusp::host_memory>(R)), cusp::invalid_input_exception);
}
void TestAINVRefusalsF64() { TestAINVRefusals<double>(); }
void TestAINVRefusalsF32() { TestAINVRefusals<float>(); }
DECLARE_UNITTEST(TestAINVRefusalsF64);
DECLARE_UNITTEST(TestAINVRefusalsF32);

// A in any of the five formats gives the factor of the CSR matrix; the apply equals W^T (d .* (W x)) formed by hand
template <typename Matrix> void TestAINVFromFormat()
{
    typedef typename Matrix::value_type V;
    const host_csr<V> C = problem<host_csr<V>>(9, 7);
    const Matrix A(C);
    const precond::bridson_ainv<V, cusp::host_memory> want(C, V(.05), 6), got(A, V(.05), 6);
    const host_csr<V> w1(want.w), w2(got.w);
    ASSERT_TRUE(w1.row_offsets == w2.row_offsets && w1.column_indices == w2.column_indices && w1.values == w2.values);
    ASSERT_TRUE(want.diagonals == got.diagonals);
    const cusp::array1d<V, cusp::host_memory> x = start_vector<V, cusp::host_memory>(C.num_rows);
    cusp::array1d<V, cusp::host_memory> y(C.num_rows), t(C.num_rows), z(C.num_rows);
    got(x, y);
    cusp::multiply(got.w, x, t);
    for (size_t i = 0; i < t.size(); i++) t[i] = t[i] * got.diagonals[i];
    cusp::multiply(got.w_t, t, z);
    ASSERT_TRUE(y == z);
}
DECLARE_SPARSE_MATRIX_UNITTEST(TestAINVFromFormat);

int main(int argc, char **argv)
{
    if (argc >= 3 && std::string(argv[1]) == "--dump") return std::string(argv[2]) == "f32" ? dump<float>() : dump<double>();
    return unittest::run_all(argc, argv);
}
