// cusp::graph::maximal_independent_set, mis_aggregate and smoothed_aggregation::mis_aggregation on host_memory.  Built and run
// by tests/test_mis_host.py.
//   test_mis_host                         runs the tests
//   test_mis_host --print A.mtx seed      for each of the five formats: stencil, size and rounds of MIS(0..3), aggregates and mis of
//                                         the square pattern in the MatrixMarket file
//   test_mis_host --levels nx ny          level sizes and the first level's aggregates of the mis_aggregation hierarchy on poisson5pt
#include "mis_check.h"

using namespace mis_check;
typedef cusp::host_memory Host;

void TestReferenceGraphsInEveryFormat()
{
    for (auto &g : reference_graphs()) {
        const result want = run(g.second, 0);
        ASSERT_TRUE(five_formats_give<Host>(g.second, 0, want));
        const size_t n = g.second.num_rows;
        ASSERT_EQUAL(want.size[0], n);                                  // k = 0: every node, no sweep
        ASSERT_EQUAL(want.rounds[0], (size_t)0);
        for (int k = 0; k < 4; k++) {
            size_t count = 0;
            for (int v : want.stencil[k]) count += v != 0;
            ASSERT_EQUAL(count, want.size[k]);
            ASSERT_EQUAL(want.stencil[k].size(), n);
        }
        ASSERT_TRUE(want.mis == want.stencil[2]);
        ASSERT_TRUE(!(run(g.second, 99) == want) || n <= 9);              // the seed matters on anything but the smallest graphs
    }
}
DECLARE_UNITTEST(TestReferenceGraphsInEveryFormat);

void TestPinnedValuesAndOverloads()
{
    const host_csr<double> A = poisson(13, 17);
    cusp::array1d<int, Host> stencil;
    cusp::array1d<char, Host> bytes;
    cusp::array1d<float, Host> reals;
    ASSERT_EQUAL(cusp::graph::maximal_independent_set(A, stencil), (size_t)88);
    ASSERT_EQUAL(cusp::graph::maximal_independent_set(A, stencil, 2), (size_t)34);
    ASSERT_EQUAL(cusp::graph::maximal_independent_set(cusp::omp::par, A, bytes), (size_t)88);
    ASSERT_EQUAL(cusp::graph::maximal_independent_set(cusp::hip::par, A, reals, 2), (size_t)34);
    size_t ones = 0;
    for (size_t i = 0; i < reals.size(); i++) ones += reals[i] == 1.0f && stencil[i] == 1;
    ASSERT_EQUAL(ones, (size_t)34);
    size_t rounds = 0;
    ASSERT_EQUAL(cusp::graph::detail::maximal_independent_set(A, stencil, 1, 0, &rounds), (size_t)88);
    ASSERT_EQUAL(rounds, (size_t)3);
    cusp::array1d<int, Host> aggregates, mis;
    agg::mis_aggregate(A, aggregates, mis);
    int top = -1, low = 0;
    for (size_t i = 0; i < aggregates.size(); i++) { top = std::max(top, aggregates[i]); low = std::min(low, aggregates[i]); }
    ASSERT_EQUAL(top, 33);
    ASSERT_EQUAL(low, 0);
    host_csr<double> R(3, 4, 0), E(0, 0, 0);
    ASSERT_THROWS(cusp::graph::maximal_independent_set(R, stencil), cusp::invalid_input_exception);
    ASSERT_THROWS(agg::mis_aggregate(R, aggregates), cusp::invalid_input_exception);
    ASSERT_EQUAL(cusp::graph::maximal_independent_set(E, stencil, 2), (size_t)0);
    ASSERT_EQUAL(stencil.size(), (size_t)0);
    host_csr<double> bad = pattern({{0, 1}, {0, 2}});                     // a column outside the matrix
    ASSERT_THROWS(cusp::graph::maximal_independent_set(bad, stencil), cusp::invalid_input_exception);
}
DECLARE_UNITTEST(TestPinnedValuesAndOverloads);

void TestMisAggregationHierarchyOnPoisson100x100()
{
    const host_csr<double> A = poisson(100, 100);
    agg::smoothed_aggregation<int, double, Host> M;
    M.mis_aggregation = true;
    M.initialize(A);
    ASSERT_TRUE(M.levels.size() >= 2);
    ASSERT_EQUAL(M.levels[1].A.num_rows, (size_t)1422);
    const cusp::array1d<double, Host> b = seeded_rhs<double, Host>(A.num_rows);
    const long with = cg_count(A, b, &M), without = cg_count(A, b, (const agg::smoothed_aggregation<int, double, Host> *)nullptr);
    std::printf("  cg iterations on 100x100: %ld with MIS(2) smoothed aggregation, %ld without; levels", with, without);
    for (auto &L : M.levels) std::printf(" %zu", L.A.num_rows);
    std::printf("\n");
    ASSERT_TRUE(with > 0 && without > 0 && with < without);
    agg::smoothed_aggregation<int, double, Host> copy(M);
    ASSERT_TRUE(copy.mis_aggregation);
    ASSERT_EQUAL(cg_count(A, b, &copy), with);
}
DECLARE_UNITTEST(TestMisAggregationHierarchyOnPoisson100x100);

// with the flag left false the hierarchy is the one built from the components with standard_aggregate, bit for bit
void TestTheFlagLeftFalseChangesNothing()
{
    const host_csr<double> A = poisson(100, 100);
    agg::smoothed_aggregation<int, double, Host> M(A), N;
    ASSERT_TRUE(!M.mis_aggregation && !N.mis_aggregation);
    N.initialize(A);
    std::vector<double> rhos;
    for (size_t i = 0; i + 1 < M.sa_levels.size(); i++) rhos.push_back(M.sa_levels[i].rho_DinvA);
    const std::vector<built_level<double, Host>> S = build<double, Host>(A, rhos, 500);
    ASSERT_EQUAL(S.size(), M.levels.size());
    ASSERT_EQUAL(M.levels.size(), (size_t)3);
    for (size_t l = 0; l < S.size(); l++) {
        ASSERT_TRUE(csr_bits_equal(M.levels[l].A, S[l].A));
        ASSERT_TRUE(csr_bits_equal(N.levels[l].A, S[l].A));
        if (l + 1 == S.size()) break;
        ASSERT_TRUE(arrays_bits_equal(M.sa_levels[l].aggregates, S[l].aggregates));
        ASSERT_TRUE(csr_bits_equal(M.levels[l].P, S[l].P));
        ASSERT_TRUE(csr_bits_equal(N.levels[l].P, S[l].P));
    }
    ASSERT_EQUAL(M.levels[1].A.num_rows, (size_t)1700);
}
DECLARE_UNITTEST(TestTheFlagLeftFalseChangesNothing);

static void print_ints(const char *name, const std::vector<int> &v)
{
    std::printf("%s", name);
    for (int x : v) std::printf(" %d", x);
    std::printf("\n");
}
template <typename Matrix> void print_result(const char *format, const Matrix &G, uint64_t seed)
{
    const result r = run(G, seed);
    std::printf("format %s\n", format);
    for (int k = 0; k < 4; k++) {
        std::printf("k %d size %zu rounds %zu\n", k, r.size[k], r.rounds[k]);
        print_ints("stencil", r.stencil[k]);
    }
    print_ints("aggregates", r.aggregates);
    print_ints("mis", r.mis);
}
static int print_formats(char **argv)
{
    cusp::coo_matrix<int, double, Host> coo;
    cusp::io::read_matrix_market_file(coo, argv[2]);
    const uint64_t seed = std::strtoull(argv[3], nullptr, 0);
    print_result("coo", coo, seed);
    print_result("csr", host_csr<double>(coo), seed);
    print_result("ell", cusp::ell_matrix<int, double, Host>(coo), seed);
    print_result("dia", cusp::dia_matrix<int, double, Host>(coo), seed);
    print_result("hyb", cusp::hyb_matrix<int, double, Host>(coo), seed);
    return 0;
}
static int print_levels(char **argv)
{
    agg::smoothed_aggregation<int, double, Host> M;
    M.mis_aggregation = true;
    M.initialize(poisson((size_t)std::atoi(argv[2]), (size_t)std::atoi(argv[3])));
    std::printf("levels");
    for (auto &L : M.levels) std::printf(" %zu", L.A.num_rows);
    std::printf("\n");
    print_ints("aggregates", cusp::detail::host_copy(M.sa_levels[0].aggregates));
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 4 && std::string(argv[1]) == "--print") return print_formats(argv);
    if (argc == 4 && std::string(argv[1]) == "--levels") return print_levels(argv);
    return unittest::run_all(argc, argv);
}
