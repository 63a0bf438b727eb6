// cusp::multiply(A, X, Y) with device_memory CSR matrices and array2d blocks: through cmi_spmm_csr_* in both orientations,
// k = 1 through the container's planned SpMV, and cusp::hip::par.on(stream) -- every result equal to the host layer's bits.
// Built and run by tests/test_spmm_gpu.py.
#include "spmm_check.h"

using namespace spmm_check;

template <typename V, typename OX, typename OY, typename M, typename HM>
void compare(const M &A, const HM &H, size_t k, bool accumulate, void *stream = nullptr)
{
    cusp::array2d<V, cusp::host_memory, OX> X(H.num_cols, k);
    cusp::array2d<V, cusp::host_memory, OY> Y0(H.num_rows, k);
    fill(X, 3 + k);
    fill(Y0, 17 + k);
    cusp::array2d<V, cusp::host_memory, OY> W = Y0;
    if (accumulate) cusp::multiply(H, X, W, cusp::identity_function<V>(), cusp::multiplies<V>(), cusp::plus<V>());
    else cusp::multiply(H, X, W);
    cusp::array2d<V, cusp::device_memory, OX> dX(X);
    cusp::array2d<V, cusp::device_memory, OY> dY(Y0);
    if (stream) {
        if (accumulate) cusp::multiply(cusp::hip::par.on(stream), A, dX, dY, cusp::identity_function<V>(), cusp::multiplies<V>(), cusp::plus<V>());
        else cusp::multiply(cusp::hip::par.on(stream), A, dX, dY);
        cusp::detail::check(cmi_stream_synchronize(stream));
    } else {
        if (accumulate) cusp::multiply(A, dX, dY, cusp::identity_function<V>(), cusp::multiplies<V>(), cusp::plus<V>());
        else cusp::multiply(A, dX, dY);
    }
    cusp::array2d<V, cusp::host_memory, OY> got(dY);
    ASSERT_TRUE(bits_equal(got, W));
}

template <typename V> void TestDeviceBlocks()
{
    cusp::csr_matrix<int, V, cusp::host_memory> P;
    cusp::gallery::poisson5pt(P, 40, 30);
    cusp::csr_matrix<int, V, cusp::host_memory> I = irregular<V>(700, 513, 9);
    for (const auto *H : {&P, &I}) {
        cusp::csr_matrix<int, V, cusp::device_memory> A(*H);
        for (size_t k : {1, 2, 3, 8, 33}) {
            compare<V, cusp::row_major, cusp::row_major>(A, *H, k, false);
            compare<V, cusp::column_major, cusp::column_major>(A, *H, k, true);
            compare<V, cusp::row_major, cusp::column_major>(A, *H, k, false);
            compare<V, cusp::column_major, cusp::row_major>(A, *H, k, true);
        }
        // a view of the device matrix (plan-less)
        compare<V, cusp::row_major, cusp::row_major>(cusp::make_csr_matrix_view(A), *H, 4, false);
    }
}
void TestDeviceBlocksF64() { TestDeviceBlocks<double>(); }
void TestDeviceBlocksF32() { TestDeviceBlocks<float>(); }
DECLARE_UNITTEST(TestDeviceBlocksF64);
DECLARE_UNITTEST(TestDeviceBlocksF32);

void TestDeviceBlockOneColumnIsThePlannedSpmv()
{
    // k = 1 with a contiguous column: the container's plan is made (the SpMV path ran), and the bits are the SpMV's
    cusp::csr_matrix<int, double, cusp::host_memory> H;
    cusp::gallery::poisson5pt(H, 200, 150);
    cusp::csr_matrix<int, double, cusp::device_memory> A(H);
    cusp::array2d<double, cusp::host_memory> X(H.num_cols, 1), Y(H.num_rows, 1, 0.0);
    fill(X, 5);
    cusp::array1d<double, cusp::host_memory> x(H.num_cols), y(H.num_rows, 0.0);
    for (size_t i = 0; i < H.num_cols; i++) x[i] = X(i, 0);
    cusp::multiply(H, x, y);
    cusp::array2d<double, cusp::device_memory> dX(X), dY(Y);
    cusp::multiply(A, dX, dY);
    ASSERT_TRUE(A.plan() != nullptr);
    cusp::array2d<double, cusp::host_memory> got(dY);
    for (size_t i = 0; i < H.num_rows; i++) ASSERT_TRUE(std::memcmp(&got(i, 0), &y[i], sizeof(double)) == 0);
}
DECLARE_UNITTEST(TestDeviceBlockOneColumnIsThePlannedSpmv);

void TestDeviceBlockStreamPolicy()
{
    void *stream = nullptr;
    cusp::detail::check(cmi_stream_create(&stream));
    cusp::csr_matrix<int, double, cusp::host_memory> H;
    cusp::gallery::poisson5pt(H, 50, 40);
    cusp::csr_matrix<int, double, cusp::device_memory> A(H);
    compare<double, cusp::row_major, cusp::row_major>(A, H, 8, false, stream);
    compare<double, cusp::column_major, cusp::column_major>(A, H, 5, true, stream);
    compare<double, cusp::row_major, cusp::row_major>(A, H, 1, false, stream);
    cusp::detail::check(cmi_stream_destroy(stream));
}
DECLARE_UNITTEST(TestDeviceBlockStreamPolicy);

void TestDeviceBlockErrors()
{
    cusp::csr_matrix<int, double, cusp::device_memory> A;
    cusp::gallery::poisson5pt(A, 4, 3);
    cusp::array2d<double, cusp::device_memory> X(12, 3, 1.0), Ybad(13, 3, 0.0), Y(12, 3, 0.0);
    ASSERT_THROWS(cusp::multiply(A, X, Ybad), cusp::invalid_input_exception);
    struct maxf { double operator()(double a, double b) const { return a > b ? a : b; } };
    ASSERT_THROWS(cusp::multiply(A, X, Y, cusp::identity_function<double>(), cusp::plus<double>(), maxf()), cusp::not_implemented_exception);
}
DECLARE_UNITTEST(TestDeviceBlockErrors);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }
