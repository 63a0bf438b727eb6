// cusp::krylov::cg_m and bicgstab_m on host_memory: the cases of multishift_check.h.  With the argument "bits" the program instead prints
// the solutions of both solvers on Poisson 10 x 10 and 7 x 5 (CSR, float and double, sigma = {0.1, 0.5, 1, 5}) as %a, one line per value:
// tests/test_multishift_host.py compares them bit for bit with the numpy restatement of tests/multishift_refs.py.
// Built and run by tests/test_multishift_host.py (also as a stand-alone program under AddressSanitizer + UndefinedBehaviorSanitizer).
#define TEST_SPACE cusp::host_memory
#define TEST_SPACE_NAME "host_memory"
#include <cstring>

#include "multishift_check.h"

using namespace multishift_check;

DECLARE_SPARSE_MATRIX_UNITTEST(TestMultiMass);
DECLARE_SPACE_UNITTEST(TestNonSymmetric);
DECLARE_SPACE_UNITTEST(TestEdgeCases);
DECLARE_SPACE_UNITTEST(TestPolicyDispatch);

template <typename Solver, typename V> void print_bits(size_t m, size_t n, const char *type)
{
    const hcsr<V> A = poisson<V>(m, n);
    const size_t N = A.num_rows;
    hvec<V> sigma(kShifts.size());
    for (size_t s = 0; s < kShifts.size(); s++) sigma[s] = V(kShifts[s]);
    const hvec<V> b(N, V(1));
    hvec<V> x(N * sigma.size(), V(0));
    cusp::monitor<V> monitor(b, 100, V(bars<V>::tolerance));
    Solver::run(A, x, b, sigma, monitor);
    std::printf("case %s %s %zux%zu iterations %zu\n", Solver::name(), type, m, n, monitor.iteration_count());
    for (size_t i = 0; i < x.size(); i++) std::printf("%a\n", (double)x[i]);
}

int main(int argc, char **argv)
{
    if (argc > 1 && std::strcmp(argv[1], "bits") == 0) {
        const size_t grids[2][2] = {{10, 10}, {7, 5}};
        for (const auto &g : grids) {
            print_bits<cg_m_solver, float>(g[0], g[1], "f32");
            print_bits<bicgstab_m_solver, float>(g[0], g[1], "f32");
            print_bits<cg_m_solver, double>(g[0], g[1], "f64");
            print_bits<bicgstab_m_solver, double>(g[0], g[1], "f64");
        }
        return 0;
    }
    return unittest::run_all(argc, argv);
}
