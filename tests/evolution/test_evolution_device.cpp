// Evolution strength of connection and cusp::gallery::diffusion on device_memory against host_memory of the same program
// (tests/test_evolution_gpu.py builds and runs this once): the measure bit for bit when rho is supplied, the refusals found on
// the device, diffusion into the five formats, and the anisotropic cg case of the host program.
#include "evolution_check.h"

using namespace evolution_check;
namespace gallery = cusp::gallery;
template <typename V> using device_csr = cusp::csr_matrix<int, V, cusp::device_memory>;

template <typename V> void compare_spaces(const host_csr<V> &A, const cusp::array1d<V, cusp::host_memory> &B, double rho, double epsilon)
{
    host_csr<V> want;
    agg::evolution_strength_of_connection(A, want, B, rho, epsilon);
    device_csr<V> dA(A), got;
    const cusp::array1d<V, cusp::device_memory> dB(B);
    agg::evolution_strength_of_connection(dA, got, dB, rho, epsilon);
    ASSERT_EQUAL(got.num_entries, want.num_entries);
    ASSERT_TRUE(csr_bits_equal(got, want));
}

// an arrow: row 0 and column 0 full, so one row is far longer than a wave while its partners hold two entries
template <typename V> host_csr<V> arrow(size_t n)
{
    host_csr<V> A(n, n, 3 * n - 2);
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        A.row_offsets[i] = (int)at;
        if (i == 0)
            for (size_t j = 0; j < n; j++) { A.column_indices[at] = (int)j; A.values[at++] = j == 0 ? V(3) : V(-1) / V(j + 1); }
        else {
            A.column_indices[at] = 0; A.values[at++] = V(-1) / V(i + 2);
            A.column_indices[at] = (int)i; A.values[at++] = V(2) + V(0.25) * V(i % 5);
        }
    }
    A.row_offsets[n] = (int)at;
    return A;
}

template <typename V> void TestDeviceEqualsHost()
{
    for (int fe = 0; fe < 2; fe++)
        for (double angle : {0.0, M_PI / 4})
            for (double epsilon : {4.0, 1.0, (double)std::numeric_limits<V>::infinity()}) {
                host_csr<V> A;
                if (fe) gallery::diffusion<gallery::FE>(A, 33, 21, 1e-3, angle);
                else gallery::diffusion<gallery::FD>(A, 33, 21, 1e-3, angle);
                cusp::array1d<V, cusp::host_memory> B(A.num_rows, V(1));
                for (size_t i = 0; i < B.size(); i += 5) B[i] = i % 2 ? V(0) : V(-0.5);
                compare_spaces<V>(A, B, 1.93, epsilon);
            }
    for (size_t n : {70, 200, 451}) compare_spaces<V>(arrow<V>(n), cusp::array1d<V, cusp::host_memory>(n, V(1)), 1.6, 4.0);
}
void TestDeviceEqualsHostF64() { TestDeviceEqualsHost<double>(); }
void TestDeviceEqualsHostF32() { TestDeviceEqualsHost<float>(); }
DECLARE_UNITTEST(TestDeviceEqualsHostF64);
DECLARE_UNITTEST(TestDeviceEqualsHostF32);

// rho estimated by the measure itself (step 3, on the device): the 7 x 5 facts; COO operands
template <typename V> void TestSevenByFiveOnTheDevice()
{
    for (int fe = 0; fe < 2; fe++) {
        device_csr<V> A, S;
        if (fe) gallery::diffusion<gallery::FE>(A, 7, 5, 1e-3, 0.0);
        else gallery::diffusion<gallery::FD>(A, 7, 5, 1e-3, 0.0);
        const cusp::array1d<V, cusp::device_memory> B(A.num_rows, V(1));
        agg::evolution_strength_of_connection(A, S, B);
        ASSERT_EQUAL(S.num_entries, (size_t)91);
        ASSERT_TRUE(diagonals_of(S) == (std::set<long>{-7, 0, 7}));
        cusp::coo_matrix<int, V, cusp::device_memory> Ac(A), Sc;
        agg::evolution_strength_of_connection(Ac, Sc, B);
        ASSERT_TRUE(csr_bits_equal(device_csr<V>(Sc), S));
    }
}
void TestSevenByFiveOnTheDeviceF64() { TestSevenByFiveOnTheDevice<double>(); }
void TestSevenByFiveOnTheDeviceF32() { TestSevenByFiveOnTheDevice<float>(); }
DECLARE_UNITTEST(TestSevenByFiveOnTheDeviceF64);
DECLARE_UNITTEST(TestSevenByFiveOnTheDeviceF32);

void TestRefusalsOnTheDevice()
{
    host_csr<double> H(3, 3, 4);
    const int offsets[4] = {0, 2, 3, 4}, columns[4] = {0, 1, 1, 2}; // (0,1) without (1,0)
    for (int i = 0; i < 4; i++) { H.row_offsets[i] = offsets[i]; H.column_indices[i] = columns[i]; H.values[i] = 1.0; }
    device_csr<double> A(H), S;
    const cusp::array1d<double, cusp::device_memory> B(3, 1.0);
    ASSERT_THROWS(agg::evolution_strength_of_connection(A, S, B, 1.5), cusp::invalid_input_exception);
    device_csr<double> rect(2, 3, 0);
    ASSERT_THROWS(agg::evolution_strength_of_connection(rect, S, B, 1.5), cusp::invalid_input_exception);
}
DECLARE_UNITTEST(TestRefusalsOnTheDevice);

template <typename Matrix> void TestDiffusionFormatsOnTheDevice()
{
    typedef typename Matrix::value_type V;
    host_csr<V> want;
    Matrix got;
    gallery::diffusion<gallery::FE>(want, 9, 6, 1e-3, 0.3);
    gallery::diffusion<gallery::FE>(got, 9, 6, 1e-3, 0.3);
    ASSERT_TRUE(csr_bits_equal(host_csr<V>(got), want));
}
#define TEST_SPACE cusp::device_memory
#define TEST_SPACE_NAME "device_memory"
DECLARE_SPARSE_MATRIX_UNITTEST(TestDiffusionFormatsOnTheDevice);

// the host program's case (see there for the figures measured on host_memory) with the hierarchy built and applied on the device
void TestSmoothedAggregationOnAnisotropy()
{
    const sa_run symmetric = anisotropic_cg<cusp::device_memory>(false), evolution = anisotropic_cg<cusp::device_memory>(true);
    print_run("symmetric strength", symmetric);
    print_run("evolution strength", evolution);
    ASSERT_TRUE(symmetric.iterations > 0 && evolution.iterations > 0);
    ASSERT_TRUE(2 * evolution.iterations <= symmetric.iterations);
}
DECLARE_UNITTEST(TestSmoothedAggregationOnAnisotropy);

int main(int argc, char **argv)
{
    if (argc >= 4 && std::string(argv[1]) == "--measure")
        return std::string(argv[2]) == "f32" ? print_measures<float, cusp::device_memory>(argc, argv) : print_measures<double, cusp::device_memory>(argc, argv);
    return unittest::run_all(argc, argv);
}
