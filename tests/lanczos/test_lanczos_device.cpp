// cusp::eigen::lanczos and cusp::blas::gemm on device_memory: the host program's unit tests (the identity / restart case and the growth case
// among them) through the fused iteration and csrc/dense.hip; "cases" runs the 16 x 12 and 33 x 31 cases fused and with $CMI_LANCZOS_FUSED=0,
// the five formats and a linear_operator once; "gemm FILE" answers the decks of the Python side, which compares them with the host program's bits.
// Built and run by tests/test_lanczos_gpu.py.
#define TEST_SPACE cusp::device_memory
#define TEST_SPACE_NAME "device_memory"
#include "lanczos_check.h"

using namespace lanczos_check;

DECLARE_SPACE_UNITTEST(TestIdentityRestarts);
DECLARE_SPACE_UNITTEST(TestDiagonalTwoByTwo);
DECLARE_SPACE_UNITTEST(TestEmptyProblems);
DECLARE_SPACE_UNITTEST(TestSpaceExhausted);
DECLARE_SPACE_UNITTEST(TestWantedCountIsClipped);
DECLARE_SPACE_UNITTEST(TestMinIterOne);
DECLARE_SPACE_UNITTEST(TestRowMajorIsRefused);
DECLARE_SPACE_UNITTEST(TestGrowthChangesNothing);
DECLARE_SPACE_UNITTEST(TestOverloads);
DECLARE_SPACE_UNITTEST(TestGemmShapes);

int main(int argc, char **argv)
{
    if (argc > 2 && std::strcmp(argv[1], "gemm") == 0) return print_gemm(argv[2]);
    if (argc > 1 && std::strcmp(argv[1], "cases") == 0) return print_cases();
    return unittest::run_all(argc, argv);
}
