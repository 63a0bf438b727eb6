// cusp::eigen on host_memory: the four spectral-radius estimators on all five formats in float and double against the exact
// values (relative error < 0.1), the Gershgorin bound against exact integers, the Hessenberg shapes (the completed column kept on
// breakdown), cusp::random_array, operators without a storage format, and cusp::relaxation::make_chebyshev_polynomial.
// Built and run by tests/test_eigen_host.py (also as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer).
#define TEST_SPACE cusp::host_memory
#define TEST_SPACE_NAME "host_memory"
#include "eigen_check.h"

using namespace eigen_check;

DECLARE_SPARSE_MATRIX_UNITTEST(TestSpectralRadiusEstimators);
DECLARE_SPARSE_MATRIX_UNITTEST(TestDisksSpectralRadius);
DECLARE_SPACE_UNITTEST(TestHessenbergShapes);
DECLARE_SPACE_UNITTEST(TestRandomArray);
DECLARE_SPACE_UNITTEST(TestLinearOperators);
DECLARE_SPACE_UNITTEST(TestChebyshevFactory);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }
