// cusp::eigen::lanczos, cusp::blas::gemm and cusp::detail::tridiagonal_eigen on host_memory: the unit tests of lanczos_check.h; with the argument
// "cases" one line per solver case of tests/lanczos_refs.py, with "gemm FILE" / "tridiag FILE" the answers to the decks of the Python side.
// Built and run by tests/test_lanczos_host.py (also as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer).
#define TEST_SPACE cusp::host_memory
#define TEST_SPACE_NAME "host_memory"
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
    if (argc > 2 && std::strcmp(argv[1], "tridiag") == 0) return print_tridiag(argv[2]);
    if (argc > 1 && std::strcmp(argv[1], "cases") == 0) return print_cases();
    return unittest::run_all(argc, argv);
}
