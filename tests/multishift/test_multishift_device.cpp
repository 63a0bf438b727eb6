// cusp::krylov::cg_m and bicgstab_m on device_memory: the host program's cases (multishift_check.h) through the fused CG-M iteration and the
// kernels of csrc/krylov_m.hip -- all five formats, float and double, both solvers; Poisson 7 x 5 makes every shift after the first
// unaligned (N = 35).  Built and run once by tests/test_multishift_gpu.py.
#define TEST_SPACE cusp::device_memory
#define TEST_SPACE_NAME "device_memory"
#include "multishift_check.h"

using namespace multishift_check;

DECLARE_SPARSE_MATRIX_UNITTEST(TestMultiMass);
DECLARE_SPACE_UNITTEST(TestNonSymmetric);
DECLARE_SPACE_UNITTEST(TestEdgeCases);
DECLARE_SPACE_UNITTEST(TestPolicyDispatch);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }
