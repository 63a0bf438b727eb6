// cusp::multiply(A, B, C) with three sparse device_memory matrices: through cmi_spgemm_csr_* (csr) and the device conversions around it (coo),
// both value types.  Device C keeps exact zeros: it equals the naive chain with zeros kept, and with its zeros removed it equals the
// host layer's C bit for bit.  The six-argument form with the standard functors, the refusal of any other functor, cusp::hip::par.on(stream).
// Built and run by tests/test_spgemm_gpu.py.
#include "spgemm_check.h"

using namespace spgemm_check;

template <typename V> void check_pair(const host_csr<V> &A, const host_csr<V> &B, void *stream = nullptr)
{
    host_csr<V> H;
    cusp::multiply(A, B, H);
    cusp::csr_matrix<int, V, cusp::device_memory> dA(A), dB(B), dC;
    if (stream) cusp::multiply(cusp::hip::par.on(stream), dA, dB, dC);
    else cusp::multiply(dA, dB, dC);
    host_csr<V> C(dC);
    ASSERT_TRUE(csr_bits_equal(C, naive(A, B, true)));
    ASSERT_TRUE(rows_strictly_ascending(C));
    ASSERT_TRUE(csr_bits_equal(without_zeros(C), H));
}

template <typename V> void TestDeviceCsrProduct()
{
    check_pair<V>(irregular<V>(300, 211, 9, 1), irregular<V>(211, 257, 7, 2));
    host_csr<V> P;
    cusp::gallery::poisson5pt(P, 30, 20);
    check_pair<V>(P, P);
    // exact cancellation and a lone -0.0 product: kept on the device as +0.0 entries, dropped on the host
    host_csr<V> A = from_rows<V>(2, 2, {{{0, V(1)}, {1, V(1)}}, {{0, V(-0.0)}}}), B = from_rows<V>(2, 2, {{{1, V(5)}, {0, V(1)}}, {{0, V(-1)}}});
    check_pair<V>(A, B);
    cusp::csr_matrix<int, V, cusp::device_memory> dA(A), dB(B), dC;
    cusp::multiply(dA, dB, dC);
    host_csr<V> C(dC);
    ASSERT_EQUAL(C.num_entries, (size_t)4); // row 0: the cancelled 0 and 5; row 1: -0.0 times both entries of B's row 0
    const V z = C.values[0], lone = C.values[2], zero = V(0);
    ASSERT_TRUE(std::memcmp(&z, &zero, sizeof(V)) == 0 && std::memcmp(&lone, &zero, sizeof(V)) == 0);
    host_csr<V> E(4, 211, 0);
    for (size_t i = 0; i <= 4; i++) E.row_offsets[i] = 0;
    check_pair<V>(E, irregular<V>(211, 9, 3, 5));
}
void TestDeviceCsrProductF64() { TestDeviceCsrProduct<double>(); }
void TestDeviceCsrProductF32() { TestDeviceCsrProduct<float>(); }
DECLARE_UNITTEST(TestDeviceCsrProductF64);
DECLARE_UNITTEST(TestDeviceCsrProductF32);

template <typename V> void TestDeviceCooProduct()
{
    host_csr<V> A = irregular<V>(120, 90, 8, 11), B = irregular<V>(90, 140, 6, 12), H;
    cusp::multiply(A, B, H);
    cusp::coo_matrix<int, V, cusp::host_memory> hA, hB;
    cusp::convert(A, hA);
    cusp::convert(B, hB);
    cusp::coo_matrix<int, V, cusp::device_memory> dA(hA), dB(hB), dC;
    cusp::multiply(dA, dB, dC);
    ASSERT_TRUE(dC.is_sorted_by_row_and_column());
    cusp::coo_matrix<int, V, cusp::host_memory> hC(dC);
    host_csr<V> C;
    cusp::convert(hC, C);
    ASSERT_TRUE(csr_bits_equal(C, naive(A, B, true)));
    ASSERT_TRUE(csr_bits_equal(without_zeros(C), H));
}
void TestDeviceCooProductF64() { TestDeviceCooProduct<double>(); }
void TestDeviceCooProductF32() { TestDeviceCooProduct<float>(); }
DECLARE_UNITTEST(TestDeviceCooProductF64);
DECLARE_UNITTEST(TestDeviceCooProductF32);

void TestDeviceSixArgumentFormAndRefusals()
{
    host_csr<double> A = irregular<double>(50, 40, 6, 21), B = irregular<double>(40, 45, 6, 22);
    cusp::csr_matrix<int, double, cusp::device_memory> dA(A), dB(B), dC, dD;
    cusp::multiply(dA, dB, dC);
    cusp::multiply(dA, dB, dD, cusp::constant_functor<double>(0.0), cusp::multiplies<double>(), cusp::plus<double>());
    ASSERT_TRUE(csr_bits_equal(host_csr<double>(dC), host_csr<double>(dD)));
    struct maxf { double operator()(double a, double b) const { return a > b ? a : b; } };
    ASSERT_THROWS(cusp::multiply(dA, dB, dD, cusp::constant_functor<double>(0.0), cusp::multiplies<double>(), maxf()), cusp::not_implemented_exception);
    ASSERT_THROWS(cusp::multiply(dA, dB, dD, cusp::constant_functor<double>(0.0), cusp::plus<double>(), cusp::plus<double>()), cusp::not_implemented_exception);
    ASSERT_THROWS(cusp::multiply(dA, dA, dD), cusp::invalid_input_exception);
    // C may be an operand
    host_csr<double> S = irregular<double>(40, 40, 5, 23);
    cusp::csr_matrix<int, double, cusp::device_memory> dS(S);
    cusp::multiply(dS, dS, dS);
    ASSERT_TRUE(csr_bits_equal(host_csr<double>(dS), naive(S, S, true)));
}
DECLARE_UNITTEST(TestDeviceSixArgumentFormAndRefusals);

void TestDeviceStreamPolicy()
{
    void *stream = nullptr;
    cusp::detail::check(cmi_stream_create(&stream));
    check_pair<double>(irregular<double>(90, 70, 9, 41), irregular<double>(70, 80, 7, 42), stream);
    check_pair<float>(irregular<float>(90, 70, 9, 43), irregular<float>(70, 80, 7, 44), stream);
    cusp::detail::check(cmi_stream_destroy(stream));
}
DECLARE_UNITTEST(TestDeviceStreamPolicy);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }
