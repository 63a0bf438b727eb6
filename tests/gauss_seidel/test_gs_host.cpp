// cusp::relaxation::gauss_seidel and sor and cusp::graph::vertex_coloring on host_memory: the cases of the reference's
// testing/gauss_seidel.cu in float and double, the colouring of the reference's matrix and of the 5-point stencil, the
// classes against a naive restatement bit for bit (symmetric and non-symmetric patterns, rows without a usable diagonal),
// and the thrown exceptions.  Built and run by tests/test_gauss_seidel_host.py (also under AddressSanitizer +
// UndefinedBehaviorSanitizer).
#define TEST_SPACE cusp::host_memory
#define TEST_SPACE_NAME "host_memory"
#include "gs_check.h"

using namespace gs_check;

DECLARE_SPACE_UNITTEST(TestGaussSeidelRelaxation);
DECLARE_SPACE_UNITTEST(TestGaussSeidelRelaxationSweeps);
DECLARE_SPACE_UNITTEST(TestVertexColoring);
DECLARE_SPACE_UNITTEST(TestAgainstNaive);
DECLARE_SPACE_UNITTEST(TestArgumentErrors);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }
