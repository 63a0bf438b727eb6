// cusp::relaxation::jacobi and polynomial on device_memory: the reference's cases on all five formats in float and double,
// every format against the naive host restatement bit for bit (cusp::multiply through the container's plan, then
// cmi_relax_jacobi_update_* / cusp::blas::axpby), x.data() unchanged by a sweep, two successive polynomial calls on one
// object, plan-less views, empty rows, empty matrices.
// Built and run by tests/test_relaxation_gpu.py.
#define TEST_SPACE cusp::device_memory
#define TEST_SPACE_NAME "device_memory"
#include "relax_check.h"

using namespace relax_check;

DECLARE_SPARSE_MATRIX_UNITTEST(TestJacobiRelaxation);
DECLARE_SPARSE_MATRIX_UNITTEST(TestJacobiRelaxationWithWeighting);
DECLARE_SPARSE_MATRIX_UNITTEST(TestPolynomialRelaxation);
DECLARE_SPARSE_MATRIX_UNITTEST(TestAgainstNaive);

template <typename V> void TestCsrViewAndEmptyRows()
{
    // a view of the device matrix (no plan) next to the container (its plan), on short rows, one of 12 entries, and empty rows
    const size_t n = 3100;
    std::vector<int> Ap(1, 0), Aj;
    for (size_t i = 0; i < n; i++) {
        if (i == 700) for (size_t j = 0; j < 12; j++) Aj.push_back((int)(j * 250 + 100 * (j >= 3)));
        else if (i % 5 != 4) { Aj.push_back((int)i); if (i + 1 < n) Aj.push_back((int)i + 1); }
        Ap.push_back((int)Aj.size());
    }
    hcsr<V> H(n, n, Aj.size());
    for (size_t i = 0; i <= n; i++) H.row_offsets[i] = Ap[i];
    for (size_t k = 0; k < Aj.size(); k++) { H.column_indices[k] = Aj[k]; H.values[k] = (V)seeded(3 + k); }
    cusp::csr_matrix<int, V, cusp::device_memory> A(H);
    auto view = cusp::make_csr_matrix_view(A);
    const hvec<V> hb = seeded_vector<V>(n, 21), hx = seeded_vector<V>(n, 22);
    cusp::array1d<V, cusp::device_memory> b(hb), x(hx), xv(hx);
    cusp::relaxation::jacobi<V, cusp::device_memory> J(A, V(0.9));
    J(A, b, x);
    J(view, b, xv);
    const hvec<V> want = naive_jacobi(H, hb, hx, V(0.9)); // (rows without a diagonal entry: inf / NaN on both sides)
    ASSERT_TRUE(bits_equal(hvec<V>(x), want));
    ASSERT_TRUE(bits_equal(hvec<V>(xv), want));
    const std::vector<V> c = {V(0.3), V(-1.1)};
    cusp::relaxation::polynomial<V, cusp::device_memory> P(A, hvec<V>(c));
    cusp::array1d<V, cusp::device_memory> px(hx);
    hvec<V> h(n, V(0));
    P(view, b, px, hvec<V>(c));
    ASSERT_TRUE(bits_equal(hvec<V>(px), naive_polynomial(H, hb, hx, c, h)));
}
void TestCsrViewAndEmptyRowsF64() { TestCsrViewAndEmptyRows<double>(); }
void TestCsrViewAndEmptyRowsF32() { TestCsrViewAndEmptyRows<float>(); }
DECLARE_UNITTEST(TestCsrViewAndEmptyRowsF64);
DECLARE_UNITTEST(TestCsrViewAndEmptyRowsF32);

void TestEmptyMatrixOnDevice()
{
    cusp::csr_matrix<int, double, cusp::device_memory> A(0, 0, 0);
    cusp::array1d<double, cusp::device_memory> b, x;
    cusp::relaxation::jacobi<double, cusp::device_memory> J(A);
    J(A, b, x);
    cusp::array1d<double, cusp::host_memory> c(2, 1.0);
    cusp::relaxation::polynomial<double, cusp::device_memory> P(A, c);
    P(A, b, x);
    ASSERT_EQUAL(x.size(), (size_t)0);
}
DECLARE_UNITTEST(TestEmptyMatrixOnDevice);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }
