// cusp::precond::aggregation::smoothed_aggregation and its parts on host_memory.  Built and run by tests/test_amg_host.py.
//   test_amg_host                                   runs the tests
//   test_amg_host --levels f64|f32 nx ny min rho... prints the hierarchy of poisson5pt(nx, ny) built with the given rho per level
//   test_amg_host --levels-mtx f64|f32 A.mtx theta min rho...  the same for the square matrix of a MatrixMarket file (entries ordered by row and column first)
#include "amg_check.h"

using namespace amg_check;

template <typename V> void TestElementwise()
{
    host_csr<V> A(2, 3, 4), B(2, 3, 3), C;
    const int ap[] = {0, 2, 4}, aj[] = {2, 0, 1, 1}, bp[] = {0, 1, 3}, bj[] = {0, 1, 2};          // row 0 of A is unsorted, row 1 holds column 1 twice
    const V ax[] = {V(1), V(2), V(3), V(4)}, bx[] = {V(2), V(7), V(-5)};
    for (int i = 0; i < 3; i++) { A.row_offsets[i] = ap[i]; B.row_offsets[i] = bp[i]; }
    for (int q = 0; q < 4; q++) { A.column_indices[q] = aj[q]; A.values[q] = ax[q]; }
    for (int q = 0; q < 3; q++) { B.column_indices[q] = bj[q]; B.values[q] = bx[q]; }
    cusp::subtract(A, B, C);                                                                        // (0,0): 2 - 2 dropped; (1,1): 3 + 4 - 7 dropped
    ASSERT_EQUAL(C.num_entries, (size_t)2);
    ASSERT_EQUAL(C.column_indices[0], 2);
    ASSERT_EQUAL(C.values[0], V(1));
    ASSERT_EQUAL(C.column_indices[1], 2);
    ASSERT_EQUAL(C.values[1], V(5));
    cusp::add(A, B, C);
    ASSERT_EQUAL(C.num_entries, (size_t)4);
    ASSERT_EQUAL(C.values[0], V(4));
    ASSERT_EQUAL(C.values[2], V(14));
    host_csr<V> D;
    cusp::elementwise(A, B, D, cusp::plus<V>());
    ASSERT_TRUE(csr_bits_equal(C, D));
    cusp::coo_matrix<int, V, cusp::host_memory> cA(A), cB(B), cC;
    cusp::add(cA, cB, cC);
    ASSERT_TRUE(csr_bits_equal(host_csr<V>(cC), C));
    host_csr<V> W(3, 3, 0);
    ASSERT_THROWS(cusp::add(A, W, C), cusp::invalid_input_exception);
}
void TestElementwiseF64() { TestElementwise<double>(); }
void TestElementwiseF32() { TestElementwise<float>(); }
DECLARE_UNITTEST(TestElementwiseF64);
DECLARE_UNITTEST(TestElementwiseF32);

void TestLevelsOfPoisson100x100()
{
    host_csr<double> A;
    cusp::gallery::poisson5pt(A, 100, 100);
    agg::smoothed_aggregation<int, double, cusp::host_memory> M(A);
    ASSERT_EQUAL(M.levels.size(), (size_t)3);
    const size_t rows[] = {10000, 1700, 192}, entries[] = {49600, 14928, 1692};
    for (size_t i = 0; i < 3; i++) {
        ASSERT_EQUAL(M.levels[i].A.num_rows, rows[i]);
        ASSERT_EQUAL(M.levels[i].A.num_entries, entries[i]);
    }
    ASSERT_TRUE(M.sa_levels[0].rho_DinvA > 1.9 && M.sa_levels[0].rho_DinvA < 2.01);
    ASSERT_TRUE(M.operator_complexity() > 1.3 && M.grid_complexity() > 1.18);
    // conditions on the iteration counts (relative residual 1e-8): converges, and in at most a third of plain cg's count
    const cusp::array1d<double, cusp::host_memory> b = seeded_rhs<double, cusp::host_memory>(A.num_rows);
    const long with = cg_count(A, b, &M), without = cg_count(A, b, (const agg::smoothed_aggregation<int, double, cusp::host_memory> *)nullptr);
    std::printf("  cg iterations on 100x100: %ld with smoothed aggregation, %ld without\n", with, without);
    ASSERT_TRUE(with > 0 && without > 0 && 3 * with <= without);
    // solve() alone converges as well
    cusp::array1d<double, cusp::host_memory> x(A.num_rows, 0.0);
    cusp::monitor<double> monitor(b, 100, 1e-8);
    M.solve(b, x, monitor);
    ASSERT_TRUE(monitor.converged());
}
DECLARE_UNITTEST(TestLevelsOfPoisson100x100);

template <typename V> void TestSmallHierarchyAndOtherFormats()
{
    host_csr<V> A;
    cusp::gallery::poisson5pt(A, 10, 10);
    agg::smoothed_aggregation<int, V, cusp::host_memory> M(A, 0.0, 20);
    ASSERT_TRUE(M.levels.size() >= 2);
    ASSERT_TRUE(M.levels.back().A.num_rows <= 20);
    cusp::coo_matrix<int, V, cusp::host_memory> coo(A);
    cusp::ell_matrix<int, V, cusp::host_memory> ell(A);
    agg::smoothed_aggregation<int, V, cusp::host_memory> Mc(coo, 0.0, 20), Me(ell, 0.0, 20);
    ASSERT_EQUAL(Mc.levels.size(), M.levels.size());
    for (size_t i = 0; i < M.levels.size(); i++) {
        ASSERT_TRUE(csr_bits_equal(Mc.levels[i].A, M.levels[i].A));
        ASSERT_TRUE(csr_bits_equal(Me.levels[i].A, M.levels[i].A));
    }
    const cusp::array1d<V, cusp::host_memory> b = seeded_rhs<V, cusp::host_memory>(A.num_rows);
    ASSERT_TRUE(cg_count(coo, b, &Mc) > 0);
}
void TestSmallHierarchyAndOtherFormatsF64() { TestSmallHierarchyAndOtherFormats<double>(); }
void TestSmallHierarchyAndOtherFormatsF32() { TestSmallHierarchyAndOtherFormats<float>(); }
DECLARE_UNITTEST(TestSmallHierarchyAndOtherFormatsF64);
DECLARE_UNITTEST(TestSmallHierarchyAndOtherFormatsF32);

void TestOneLevelIsTheLuSolve()
{
    host_csr<double> A;
    cusp::gallery::poisson5pt(A, 6, 5);
    agg::smoothed_aggregation<int, double, cusp::host_memory> M(A);       // 30 rows <= 500
    ASSERT_EQUAL(M.levels.size(), (size_t)1);
    const cusp::array1d<double, cusp::host_memory> b = seeded_rhs<double, cusp::host_memory>(30);
    cusp::array1d<double, cusp::host_memory> x(30, 0.0), y(30, 0.0), r(30);
    M(b, x);
    cusp::detail::lu_solver<double, cusp::host_memory> lu(A);
    lu(b, y);
    ASSERT_TRUE(arrays_bits_equal(x, y));
    cusp::multiply(A, x, r);
    for (size_t i = 0; i < 30; i++) ASSERT_TRUE(std::abs(r[i] - b[i]) < 1e-13);
    host_csr<double> Z(3, 3, 0);
    for (int i = 0; i <= 3; i++) Z.row_offsets[i] = 0;
    ASSERT_THROWS((cusp::detail::lu_solver<double, cusp::host_memory>(Z)), cusp::runtime_exception);
    host_csr<double> W(3, 4, 0);
    ASSERT_THROWS((agg::smoothed_aggregation<int, double, cusp::host_memory>(W)), cusp::invalid_input_exception);
}
DECLARE_UNITTEST(TestOneLevelIsTheLuSolve);

template <typename V> void print_csr(const char *name, const host_csr<V> &m)
{
    std::printf("%s %zu %zu %zu\n", name, m.num_rows, m.num_cols, m.num_entries);
    for (size_t i = 0; i <= m.num_rows; i++) std::printf("%d ", (int)m.row_offsets[i]);
    std::printf("\n");
    for (size_t q = 0; q < m.num_entries; q++) {
        const V v = m.values[q];
        uint64_t bits = 0;
        std::memcpy(&bits, &v, sizeof(V));
        std::printf("%d %" PRIx64 "\n", (int)m.column_indices[q], bits);
    }
}
template <typename V> int print_built(const std::vector<built_level<V, cusp::host_memory>> &L)
{
    std::printf("levels %zu\n", L.size());
    for (size_t l = 0; l < L.size(); l++) {
        print_csr("A", L[l].A);
        if (l + 1 == L.size()) break;
        std::printf("aggregates %zu\n", L[l].aggregates.size());
        for (size_t i = 0; i < L[l].aggregates.size(); i++) std::printf("%d ", (int)L[l].aggregates[i]);
        std::printf("\n");
        print_csr("P", L[l].P);
    }
    return 0;
}
template <typename V> int print_levels(int argc, char **argv)
{
    host_csr<V> A;
    cusp::gallery::poisson5pt(A, (size_t)std::atoi(argv[3]), (size_t)std::atoi(argv[4]));
    std::vector<double> rhos;
    for (int i = 6; i < argc; i++) rhos.push_back(std::atof(argv[i]));
    return print_built(build<V, cusp::host_memory>(A, rhos, (size_t)std::atoi(argv[5])));
}
template <typename V> int print_levels_mtx(int argc, char **argv)
{
    cusp::coo_matrix<int, V, cusp::host_memory> coo;
    cusp::io::read_matrix_market_file(coo, argv[3]);
    coo.sort_by_row_and_column();
    host_csr<V> A(coo);
    std::vector<double> rhos;
    for (int i = 6; i < argc; i++) rhos.push_back(std::atof(argv[i]));
    return print_built(build<V, cusp::host_memory>(A, rhos, (size_t)std::atoi(argv[5]), std::atof(argv[4])));
}

int main(int argc, char **argv)
{
    if (argc >= 6 && std::string(argv[1]) == "--levels") return std::string(argv[2]) == "f32" ? print_levels<float>(argc, argv) : print_levels<double>(argc, argv);
    if (argc >= 6 && std::string(argv[1]) == "--levels-mtx") return std::string(argv[2]) == "f32" ? print_levels_mtx<float>(argc, argv) : print_levels_mtx<double>(argc, argv);
    return unittest::run_all(argc, argv);
}
