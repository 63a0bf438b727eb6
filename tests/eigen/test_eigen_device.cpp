// cusp::eigen on device_memory: the host program's matrices and criterion on all five formats in float and double through the fused
// device sequences (cmi_{csr,ell,dia}_abs_row_sums_*, cmi_random_fill_*, cmi_blas_axpy_dot_* + cmi_blas_scal_recip_*), estimate_rho_Dinv_A,
// make_chebyshev_polynomial, cusp::random_array copied to the host and to the device with equal bits, and the Hessenberg shape of the
// device arnoldi.  Built and run by tests/test_eigen_gpu.py.
#define TEST_SPACE cusp::device_memory
#define TEST_SPACE_NAME "device_memory"
#include "eigen_check.h"

using namespace eigen_check;

DECLARE_SPARSE_MATRIX_UNITTEST(TestSpectralRadiusEstimators);
DECLARE_SPARSE_MATRIX_UNITTEST(TestDisksSpectralRadius);
DECLARE_SPACE_UNITTEST(TestHessenbergShapes);
DECLARE_SPACE_UNITTEST(TestRandomArray);
DECLARE_SPACE_UNITTEST(TestLinearOperators);
DECLARE_SPACE_UNITTEST(TestChebyshevFactory);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }
