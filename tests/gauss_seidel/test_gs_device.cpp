// cusp::relaxation::gauss_seidel and sor and cusp::graph::vertex_coloring on device_memory: the reference's cases in float
// and double, the colourings, the classes against the naive host restatement bit for bit (one cmi_csr_gauss_seidel_colour_*
// call per colour; colours whose rows depend on one another through the parked two-launch form), x.data() unchanged by a
// sweep, copies between the memory spaces, the thrown exceptions, an empty matrix.
// Built and run by tests/test_gauss_seidel_gpu.py.
#define TEST_SPACE cusp::device_memory
#define TEST_SPACE_NAME "device_memory"
#include "gs_check.h"

using namespace gs_check;

DECLARE_SPACE_UNITTEST(TestGaussSeidelRelaxation);
DECLARE_SPACE_UNITTEST(TestGaussSeidelRelaxationSweeps);
DECLARE_SPACE_UNITTEST(TestVertexColoring);
DECLARE_SPACE_UNITTEST(TestAgainstNaive);
DECLARE_SPACE_UNITTEST(TestArgumentErrors);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }
