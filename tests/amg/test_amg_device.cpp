// cusp::precond::aggregation::smoothed_aggregation on device_memory against the host_memory classes of the same program.
// Built and run once, in a child process, by tests/test_amg_gpu.py.
#include "amg_check.h"

using namespace amg_check;
typedef cusp::device_memory Dev;
typedef cusp::host_memory Host;

// Components called with the HOST's rho: aggregates, sizes and entry counts identical, every matrix bit for bit; each coarse
// operator equals R (A P) recomputed on the host from the device's own P (the device product keeps exact-zero sums, the host
// product drops them: compared with the zeros removed, and counted)
template <typename V> void compare_built(const host_csr<V> &A, const std::vector<double> &rhos, size_t min_level_size, double theta, size_t *cancelled = nullptr)
{
    const std::vector<built_level<V, Host>> H = build<V, Host>(A, rhos, min_level_size, theta);
    cusp::csr_matrix<int, V, Dev> dA(A);
    const std::vector<built_level<V, Dev>> D = build<V, Dev>(dA, rhos, min_level_size, theta);
    ASSERT_EQUAL(D.size(), H.size());
    for (size_t l = 0; l < H.size(); l++) {
        ASSERT_EQUAL(D[l].A.num_rows, H[l].A.num_rows);
        ASSERT_EQUAL(D[l].A.num_entries, H[l].A.num_entries);
        ASSERT_TRUE(csr_bits_equal(D[l].A, H[l].A));
        ASSERT_TRUE(arrays_bits_equal(D[l].B, H[l].B));
        if (l + 1 == H.size()) break;
        ASSERT_TRUE(arrays_bits_equal(D[l].aggregates, H[l].aggregates));
        ASSERT_TRUE(csr_bits_equal(D[l].S, H[l].S));
        ASSERT_TRUE(csr_bits_equal(D[l].T, H[l].T));
        ASSERT_TRUE(csr_bits_equal(D[l].P, H[l].P));
        ASSERT_TRUE(csr_bits_equal(D[l].R, H[l].R));
        host_csr<V> hP(D[l].P), hA(D[l].A), hR, AP, RAP;
        agg::form_restriction(hP, hR);
        cusp::multiply(hA, hP, AP);
        cusp::multiply(hR, AP, RAP);
        ASSERT_TRUE(csr_bits_equal(D[l + 1].A, RAP));
        if (cancelled) *cancelled += structural_product_entries(hA, hP) - AP.num_entries + structural_product_entries(hR, AP) - RAP.num_entries;
    }
}
template <typename V> void compare_components(size_t nx, size_t ny, size_t min_level_size)
{
    host_csr<V> A;
    cusp::gallery::poisson5pt(A, nx, ny);
    agg::smoothed_aggregation<int, V, Host> M(A, 0.0, min_level_size);
    std::vector<double> rhos;
    for (size_t i = 0; i + 1 < M.sa_levels.size(); i++) rhos.push_back(M.sa_levels[i].rho_DinvA);
    compare_built(A, rhos, min_level_size, 0.0);
    ASSERT_EQUAL((build<V, Host>(A, rhos, min_level_size).size()), M.levels.size());
}
// An irregular pattern that is not symmetric, with isolated nodes (aggregate -1, empty rows of T), empty rows, a threshold that cuts, and values
// and rho chosen so that sums cancel EXACTLY in A P and R (A P): the device products keep such zeros and galerkin_product must drop them
template <typename V> void TestComponentsIrregular()
{
    const host_csr<V> A = irregular_square<V>(1500, 9, 77, false);
    size_t cancelled = 0;
    compare_built(A, std::vector<double>(4, 4.0 / 3.0), 30, 0.25, &cancelled);
    std::printf("  exact-zero sums dropped from the Galerkin products: %zu\n", cancelled);
    ASSERT_TRUE(cancelled > 0);
    compare_built(A, std::vector<double>(4, 1.6), 30, 0.0);
}
void TestComponentsIrregularF64() { TestComponentsIrregular<double>(); }
void TestComponentsIrregularF32() { TestComponentsIrregular<float>(); }
DECLARE_UNITTEST(TestComponentsIrregularF64);
DECLARE_UNITTEST(TestComponentsIrregularF32);
void TestComponents100x100Min500F64() { compare_components<double>(100, 100, 500); }
void TestComponents100x100Min50F64() { compare_components<double>(100, 100, 50); }
void TestComponents100x100Min500F32() { compare_components<float>(100, 100, 500); }
void TestComponents10x10Min20F64() { compare_components<double>(10, 10, 20); }
void TestComponents10x10Min20F32() { compare_components<float>(10, 10, 20); }
DECLARE_UNITTEST(TestComponents100x100Min500F64);
DECLARE_UNITTEST(TestComponents100x100Min50F64);
DECLARE_UNITTEST(TestComponents100x100Min500F32);
DECLARE_UNITTEST(TestComponents10x10Min20F64);
DECLARE_UNITTEST(TestComponents10x10Min20F32);

// The class itself: the same levels as the host class, and the conditions on cg's iteration counts (relative residual 1e-8)
template <typename Matrix> void class_and_cg(const Matrix &dA, const host_csr<double> &A, size_t min_level_size)
{
    agg::smoothed_aggregation<int, double, Host> MH(A, 0.0, min_level_size);
    agg::smoothed_aggregation<int, double, Dev> MD(dA, 0.0, min_level_size);
    ASSERT_EQUAL(MD.levels.size(), MH.levels.size());
    for (size_t l = 0; l < MH.levels.size(); l++) {
        ASSERT_EQUAL(MD.levels[l].A.num_rows, MH.levels[l].A.num_rows);
        ASSERT_EQUAL(MD.levels[l].A.num_entries, MH.levels[l].A.num_entries);
        ASSERT_TRUE(arrays_bits_equal(MD.levels[l].A.column_indices, MH.levels[l].A.column_indices));
        if (l + 1 < MH.levels.size()) ASSERT_TRUE(arrays_bits_equal(MD.sa_levels[l].aggregates, MH.sa_levels[l].aggregates));
    }
    const cusp::array1d<double, Host> hb = seeded_rhs<double, Host>(A.num_rows);
    const cusp::array1d<double, Dev> db(hb);
    const long host_count = cg_count(A, hb, &MH), device_count = cg_count(dA, db, &MD);
    const long plain = cg_count(dA, db, (const agg::smoothed_aggregation<int, double, Dev> *)nullptr);
    std::printf("  cg iterations (%zu rows, min_level_size %zu): device preconditioner %ld, host preconditioner %ld, none %ld\n", A.num_rows, min_level_size,
                device_count, host_count, plain);
    ASSERT_TRUE(device_count > 0);
    ASSERT_TRUE(device_count <= host_count + 2);
    ASSERT_TRUE(3 * device_count <= plain);
    // the cross-space copy gives a working host preconditioner
    agg::smoothed_aggregation<int, double, Host> copy(MD);
    ASSERT_TRUE(cg_count(A, hb, &copy) <= host_count + 2);
}
void TestClassAndCgCsr()
{
    host_csr<double> A;
    cusp::gallery::poisson5pt(A, 100, 100);
    class_and_cg(cusp::csr_matrix<int, double, Dev>(A), A, 500);
    class_and_cg(cusp::csr_matrix<int, double, Dev>(A), A, 50);
}
void TestClassAndCgCoo()
{
    host_csr<double> A;
    cusp::gallery::poisson5pt(A, 100, 100);
    class_and_cg(cusp::coo_matrix<int, double, Dev>(A), A, 500);
}
void TestClassAndCgEll()
{
    host_csr<double> A;
    cusp::gallery::poisson5pt(A, 100, 100);
    class_and_cg(cusp::ell_matrix<int, double, Dev>(A), A, 500);
}
DECLARE_UNITTEST(TestClassAndCgCsr);
DECLARE_UNITTEST(TestClassAndCgCoo);
DECLARE_UNITTEST(TestClassAndCgEll);

void TestOneLevelIsTheLuSolve()
{
    host_csr<double> A;
    cusp::gallery::poisson5pt(A, 6, 5);
    cusp::csr_matrix<int, double, Dev> dA(A);
    agg::smoothed_aggregation<int, double, Dev> M(dA);
    ASSERT_EQUAL(M.levels.size(), (size_t)1);
    const cusp::array1d<double, Host> hb = seeded_rhs<double, Host>(30);
    cusp::array1d<double, Dev> b(hb), x(30, 0.0);
    cusp::array1d<double, Host> y(30, 0.0);
    M(b, x);
    cusp::detail::lu_solver<double, Host> lu(A);
    lu(hb, y);
    ASSERT_TRUE(arrays_bits_equal(x, y));
}
DECLARE_UNITTEST(TestOneLevelIsTheLuSolve);

template <typename V> void TestDeviceElementwise()
{
    host_csr<V> A, B;
    cusp::gallery::poisson5pt(A, 13, 9);
    cusp::gallery::poisson5pt(B, 13, 9);
    for (size_t q = 0; q < B.num_entries; q++) B.values[q] = (q % 3 == 0) ? A.values[q] : V(0.37) * V(q % 7);
    std::swap(B.column_indices[0], B.column_indices[1]); // row 0 unsorted: the device call reports it and the host path runs
    std::swap(B.values[0], B.values[1]);
    host_csr<V> hC, hD;
    cusp::csr_matrix<int, V, Dev> dA(A), dB(B), dC;
    cusp::subtract(A, B, hC);
    cusp::subtract(dA, dB, dC);
    ASSERT_TRUE(csr_bits_equal(dC, hC));
    cusp::add(A, A, hD);
    cusp::add(dA, dA, dC);
    ASSERT_TRUE(csr_bits_equal(dC, hD));
    cusp::coo_matrix<int, V, Dev> cA(dA), cC;
    cusp::add(cA, cA, cC);
    ASSERT_TRUE(csr_bits_equal(host_csr<V>(cC), hD));
}
void TestDeviceElementwiseF64() { TestDeviceElementwise<double>(); }
void TestDeviceElementwiseF32() { TestDeviceElementwise<float>(); }
DECLARE_UNITTEST(TestDeviceElementwiseF64);
DECLARE_UNITTEST(TestDeviceElementwiseF32);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }
