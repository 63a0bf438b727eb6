// cusp::graph::breadth_first_search, pseudo_peripheral_vertex, symmetric_rcm, connected_components and cusp::permutation_matrix
// on host_memory.  Built and run by tests/test_graph_host.py.
//   test_graph_host                          runs the tests
//   test_graph_host --print A.mtx src start  for each of the five formats: what graph_check::run gathers for the square pattern in
//                                            the MatrixMarket file
#include "graph_check.h"

using namespace graph_check;
typedef cusp::host_memory Host;

void TestReferenceGraphsInEveryFormat()
{
    for (auto &g : reference_graphs()) {
        const host_csr<double> A = numbered(g.second);
        const long n = (long)A.num_rows;
        for (long src : {0l, n / 2}) {
            const result want = run(A, src, src);
            if (!five_formats_give<Host>(A, src, src, want)) std::printf("  differs: %s from %ld\n", g.first.c_str(), src);
            ASSERT_TRUE(five_formats_give<Host>(A, src, src, want));
            ASSERT_TRUE(want.permuted && permuted_by_hand(A, want));
            if (n <= 9) ASSERT_TRUE(run(cusp::dia_matrix<int, double, Host>(A), src, src).permuted);
            std::vector<int> sorted(want.permutation);
            std::sort(sorted.begin(), sorted.end());
            for (long i = 0; i < n; i++) ASSERT_EQUAL(sorted[i], (int)i);
            for (long i = 0; i < n; i++) ASSERT_EQUAL(want.scattered[(size_t)want.permutation[i]], 0.5 + (double)i);
            for (long i = 0; i < n; i++) ASSERT_EQUAL(want.gathered[i], 0.5 + (double)want.permutation[i]);
        }
    }
}
DECLARE_UNITTEST(TestReferenceGraphsInEveryFormat);

void TestPinnedValuesAndOverloads()
{
    const host_csr<double> A = poisson(13, 17);
    cusp::array1d<int, Host> labels;
    cusp::array1d<float, Host> reals;
    cusp::graph::breadth_first_search(A, 0, labels);
    ASSERT_EQUAL(labels[220], 28);
    cusp::graph::breadth_first_search(cusp::omp::par, A, 0, reals, false);
    ASSERT_EQUAL(reals[0], -2.0f);
    ASSERT_EQUAL(reals[14], 1.0f);                                       // of 1 and 13 the smaller
    ASSERT_EQUAL(cusp::graph::pseudo_peripheral_vertex(A), 0);                // 0 -> 220 -> 0: the depth stays 28
    ASSERT_EQUAL(cusp::graph::pseudo_peripheral_vertex(cusp::hip::par, A, labels), 0);
    ASSERT_EQUAL(labels[0], 28);
    int searches = 0;
    ASSERT_EQUAL(cusp::graph::detail::pseudo_peripheral_vertex(A, labels, 110, &searches), 0);
    ASSERT_EQUAL(searches, 3);
    cusp::permutation_matrix<int, Host> P, I(5);
    cusp::graph::symmetric_rcm(A, P);
    cusp::graph::symmetric_rcm(cusp::hip::par, A, P);
    ASSERT_EQUAL(P.num_rows, (size_t)221);
    ASSERT_EQUAL(P.permutation[220], 0);
    ASSERT_EQUAL(P.permutation[0], 220);
    ASSERT_EQUAL(I.permutation[4], 4);
    ASSERT_EQUAL(I.num_entries, (size_t)5);
    const cusp::permutation_matrix<int, Host> Q(221, P.permutation), R(Q);
    ASSERT_TRUE(R.permutation == P.permutation);
    ASSERT_EQUAL(cusp::graph::connected_components(A, labels), (size_t)1);
    ASSERT_EQUAL(cusp::graph::connected_components(cusp::hip::par, pattern(std::vector<std::vector<int>>(6)), reals), (size_t)6);
    ASSERT_EQUAL(reals[5], 5.0f);
    ASSERT_EQUAL(cusp::graph::connected_components(pattern({{0, 1}, {0, 1}, {2, 3}, {2, 3}}), labels), (size_t)2);
    ASSERT_EQUAL(labels[1], 0);
    ASSERT_EQUAL(labels[2], 1);
}
DECLARE_UNITTEST(TestPinnedValuesAndOverloads);

void TestRefusals()
{
    cusp::array1d<int, Host> labels(3, 7);
    cusp::permutation_matrix<int, Host> P;
    host_csr<double> R(3, 4, 0), E(0, 0, 0);
    ASSERT_THROWS(cusp::graph::breadth_first_search(R, 0, labels), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::pseudo_peripheral_vertex(R), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::symmetric_rcm(R, P), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::connected_components(R, labels), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::breadth_first_search(E, 0, labels), cusp::invalid_input_exception);   // no vertex: no source
    ASSERT_EQUAL(cusp::graph::connected_components(E, labels), (size_t)0);
    labels = cusp::array1d<int, Host>(3, 7);
    const host_csr<double> bad = pattern({{1}, {0, 2}, {1, 9}, {3}});       // from 0 the search reaches row 2, from 3 it does not
    ASSERT_THROWS(cusp::graph::breadth_first_search(bad, 0, labels), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::breadth_first_search(bad, 4, labels), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::breadth_first_search(bad, -1, labels), cusp::invalid_input_exception);
    ASSERT_EQUAL(labels.size(), (size_t)3);
    ASSERT_EQUAL(labels[2], 7);                                          // left as it was
    cusp::graph::breadth_first_search(bad, 3, labels);
    ASSERT_TRUE(cusp::detail::host_copy(labels) == std::vector<int>({-1, -1, -1, 0}));
    host_csr<double> skip = pattern({{1, -1}, {0, 2, 2}, {1}});           // -1 is skipped
    cusp::graph::breadth_first_search(skip, 0, labels);
    ASSERT_TRUE(cusp::detail::host_copy(labels) == std::vector<int>({0, 1, 2}));
    cusp::permutation_matrix<int, Host> wrong(3);
    wrong.permutation[1] = 3;
    host_csr<double> A = pattern({{0, 1}, {1}, {2}});
    cusp::array1d<double, Host> x(3, 1.0), y(3, 0.0), z(4, 0.0);
    const cusp::permutation_matrix<int, Host> four(4);
    ASSERT_THROWS(cusp::multiply(wrong, x, y), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::multiply(x, wrong, y), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::multiply(four, x, y), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::multiply(x, cusp::permutation_matrix<int, Host>(3), z), cusp::invalid_input_exception);
    ASSERT_THROWS(four.symmetric_permute(A), cusp::invalid_input_exception);
}
DECLARE_UNITTEST(TestRefusals);

static void print_ints(const char *name, const std::vector<int> &v)
{
    std::printf("%s", name);
    for (int x : v) std::printf(" %d", x);
    std::printf("\n");
}
template <typename Matrix> void print_result(const char *format, const Matrix &G, long src, long start)
{
    const result r = run(G, src, start);
    std::printf("format %s\n", format);
    std::printf("search %zu %d\n", r.reached, r.depth);
    print_ints("levels", r.levels);
    print_ints("preds", r.preds);
    std::printf("peripheral %ld %d %ld\n", r.vertex, r.searches, r.rcm_vertex);
    print_ints("last_levels", r.last_levels);
    print_ints("permutation", r.permutation);
    std::printf("count %zu\n", r.count);
    print_ints("components", r.components);
    print_ints("rows", r.rows);
    print_ints("cols", r.cols);
    std::printf("values");
    for (double v : r.values) std::printf(" %.17g", v);
    std::printf("\n");
}
static int print_formats(char **argv)
{
    cusp::coo_matrix<int, double, Host> coo;
    cusp::io::read_matrix_market_file(coo, argv[2]);
    const long src = std::atol(argv[3]), start = std::atol(argv[4]);
    print_result("coo", coo, src, start);
    print_result("csr", host_csr<double>(coo), src, start);
    print_result("ell", cusp::ell_matrix<int, double, Host>(coo), src, start);
    print_result("dia", cusp::dia_matrix<int, double, Host>(coo), src, start);
    print_result("hyb", cusp::hyb_matrix<int, double, Host>(coo), src, start);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc == 5 && std::string(argv[1]) == "--print") return print_formats(argv);
    return unittest::run_all(argc, argv);
}
