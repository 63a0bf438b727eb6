// cusp::eigen::lobpcg on device_memory: the host program's unit tests and cases (lobpcg_check.h) through the fused iteration and the kernels of
// csrc/lobpcg.hip -- all five formats, float and double; "cases" runs every case fused, fused again and with $CMI_LOBPCG_FUSED=0.
// Built and run by tests/test_lobpcg_gpu.py.
#define TEST_SPACE cusp::device_memory
#define TEST_SPACE_NAME "device_memory"
#include "lobpcg_check.h"

using namespace lobpcg_check;

DECLARE_SPARSE_MATRIX_UNITTEST(TestFormats);
DECLARE_SPACE_UNITTEST(TestLinearOperator);
DECLARE_SPACE_UNITTEST(TestArray2dAndOverloads);
DECLARE_SPACE_UNITTEST(TestIterationCap);
DECLARE_SPACE_UNITTEST(TestBreakdownRule);
DECLARE_SPACE_UNITTEST(TestShapes);

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "cases") == 0) return print_cases();
    return unittest::run_all(argc, argv);
}
