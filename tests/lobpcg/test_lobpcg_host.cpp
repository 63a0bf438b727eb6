// cusp::eigen::lobpcg on host_memory: the unit tests of lobpcg_check.h; with the argument "cases" the program instead prints one line per solver
// case of tests/lobpcg_refs.py, which tests/test_lobpcg_host.py checks against the exact eigenvalues and the restatement's iteration counts.
// With "sygv FILE" it reads pairs (n, then n * n values of A and of B per line) and prints cusp::detail::sygv_small's answer as %a, which the
// Python side compares bit for bit with the numpy restatement of the small solver.
// Built and run by tests/test_lobpcg_host.py (also as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer).
#define TEST_SPACE cusp::host_memory
#define TEST_SPACE_NAME "host_memory"
#include "lobpcg_check.h"

using namespace lobpcg_check;

DECLARE_SPARSE_MATRIX_UNITTEST(TestFormats);
DECLARE_SPACE_UNITTEST(TestLinearOperator);
DECLARE_SPACE_UNITTEST(TestArray2dAndOverloads);
DECLARE_SPACE_UNITTEST(TestIterationCap);
DECLARE_SPACE_UNITTEST(TestBreakdownRule);
DECLARE_SPACE_UNITTEST(TestShapes);

static int print_sygv(const char *path)
{
    std::FILE *f = std::fopen(path, "r");
    if (!f) return 2;
    int n;
    while (std::fscanf(f, "%d", &n) == 1 && n >= 1 && n <= 3) {
        double A[9], B[9], w[3], Z[9];
        for (int k = 0; k < n * n; k++) if (std::fscanf(f, "%la", &A[k]) != 1) return 2;
        for (int k = 0; k < n * n; k++) if (std::fscanf(f, "%la", &B[k]) != 1) return 2;
        const bool ok = cusp::detail::sygv_small(n, A, B, w, Z);
        std::printf("%d", (int)ok);
        for (int k = 0; ok && k < n; k++) std::printf(" %a", w[k]);
        for (int k = 0; ok && k < n * n; k++) std::printf(" %a", Z[k]);
        std::printf("\n");
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 2 && std::strcmp(argv[1], "sygv") == 0) return print_sygv(argv[2]);
    if (argc > 1 && std::strcmp(argv[1], "cases") == 0) return print_cases();
    return unittest::run_all(argc, argv);
}
