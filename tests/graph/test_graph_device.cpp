// cusp::graph::breadth_first_search, pseudo_peripheral_vertex, symmetric_rcm, connected_components and cusp::permutation_matrix
// on device_memory against the host_memory paths of the same program.  Built and run once, in a child process, by
// tests/test_graph_gpu.py.
#include "graph_check.h"

using namespace graph_check;
typedef cusp::device_memory Dev;
typedef cusp::host_memory Host;

// labels, counts, vertex, ordering, components, the permuted matrix entry for entry and both vector products: the five device
// formats against the host CSR path
void TestDeviceEqualsHostInEveryFormat()
{
    for (auto &g : reference_graphs()) {
        const host_csr<double> A = numbered(g.second);
        const long n = (long)A.num_rows;
        for (long src : {0l, n / 2}) {
            const result want = run(A, src, n - 1 - src);
            if (!five_formats_give<Dev>(A, src, n - 1 - src, want)) std::printf("  differs: %s from %ld\n", g.first.c_str(), src);
            ASSERT_TRUE(five_formats_give<Dev>(A, src, n - 1 - src, want));
            ASSERT_TRUE(want.permuted && permuted_by_hand(A, want));
        }
    }
}
DECLARE_UNITTEST(TestDeviceEqualsHostInEveryFormat);

// directed edges, isolated vertices, empty rows, repeated columns, several components; explicit -1 columns in CSR
void TestIrregularPatterns()
{
    const host_csr<double> A = numbered(amg_check::irregular_square<double>(1500, 9, 77));
    const cusp::csr_matrix<int, double, Dev> dA(A);
    for (long src : {0l, 5l, 700l, 1499l}) {
        const result want = run(A, src, src);
        ASSERT_TRUE(run(dA, src, src) == want);
        ASSERT_TRUE(want.count > 1);
    }
    host_csr<double> S = pattern({{3, 1, 1, 0}, {-1, 2, 0}, {2, 2, 1, -1}, {0, 4}, {}, {6, 5, -1, 4}, {5, 7, 7}, {8, 6}, {7, -1}, {10, 9}, {9}, {}});
    const cusp::csr_matrix<int, double, Dev> dS(S);
    cusp::array1d<int, Dev> labels, components;
    cusp::array1d<int, Host> on_host, host_components;
    for (int src = 0; src < 12; src++)
        for (bool mark : {true, false}) {
            cusp::graph::breadth_first_search(dS, src, labels, mark);
            cusp::graph::breadth_first_search(S, src, on_host, mark);
            ASSERT_TRUE(cusp::detail::host_copy(labels) == cusp::detail::host_copy(on_host));
        }
    ASSERT_EQUAL(cusp::graph::connected_components(dS, components), cusp::graph::connected_components(S, host_components));
    ASSERT_TRUE(cusp::detail::host_copy(components) == cusp::detail::host_copy(host_components));
}
DECLARE_UNITTEST(TestIrregularPatterns);

void TestComponentsAndOverloads()
{
    cusp::array1d<int, Dev> labels;
    cusp::array1d<float, Dev> reals;
    cusp::array1d<int, Host> on_host;
    const cusp::coo_matrix<int, float, Dev> two(pattern({{0, 1}, {0, 1}, {2, 3}, {2, 3}}));
    ASSERT_EQUAL(cusp::graph::connected_components(two, labels), (size_t)2);
    ASSERT_TRUE(cusp::detail::host_copy(labels) == std::vector<int>({0, 0, 1, 1}));
    const cusp::csr_matrix<int, double, Dev> six(pattern(std::vector<std::vector<int>>(6)));
    ASSERT_EQUAL(cusp::graph::connected_components(cusp::hip::par, six, on_host), (size_t)6);
    ASSERT_TRUE(cusp::detail::host_copy(on_host) == std::vector<int>({0, 1, 2, 3, 4, 5}));
    const cusp::csr_matrix<int, float, Dev> P(poisson(13, 17));
    cusp::graph::breadth_first_search(P, 0, labels);
    ASSERT_EQUAL((int)labels[220], 28);
    cusp::graph::breadth_first_search(cusp::hip::par, P, 0, reals, false);
    ASSERT_EQUAL((float)reals[14], 1.0f);
    ASSERT_EQUAL(cusp::graph::pseudo_peripheral_vertex(P), 0);
    ASSERT_EQUAL(cusp::graph::pseudo_peripheral_vertex(cusp::hip::par, P, on_host), 0);
    ASSERT_EQUAL(on_host[0], 28);
    int searches = 0;
    ASSERT_EQUAL(cusp::graph::detail::pseudo_peripheral_vertex(P, labels, 110, &searches), 0);
    ASSERT_EQUAL(searches, 3);
    cusp::permutation_matrix<int, Dev> Q;
    cusp::graph::symmetric_rcm(cusp::hip::par, P, Q);
    const cusp::permutation_matrix<int, Host> H(Q);
    ASSERT_EQUAL(H.num_rows, (size_t)221);
    ASSERT_EQUAL(H.permutation[220], 0);
    ASSERT_EQUAL(H.permutation[0], 220);
    ASSERT_EQUAL(cusp::graph::connected_components(P, labels), (size_t)1);
    // float and int vectors through the permutation
    std::vector<float> xf(221);
    std::vector<int> xi(221);
    for (int i = 0; i < 221; i++) { xf[i] = 0.25f * (float)i; xi[i] = 1000 - i; }
    const cusp::array1d<float, Dev> dxf(xf);
    const cusp::array1d<int, Dev> dxi(xi);
    cusp::array1d<float, Dev> yf(221);
    cusp::array1d<int, Dev> yi(221);
    cusp::multiply(Q, dxf, yf);
    cusp::multiply(dxi, Q, yi);
    const std::vector<float> gf = cusp::detail::host_copy(yf);
    const std::vector<int> gi = cusp::detail::host_copy(yi);
    for (int i = 0; i < 221; i++) {
        ASSERT_EQUAL(gf[i], xf[(size_t)H.permutation[i]]);
        ASSERT_EQUAL(gi[(size_t)H.permutation[i]], xi[i]);
    }
}
DECLARE_UNITTEST(TestComponentsAndOverloads);

void TestRefusals()
{
    cusp::array1d<int, Dev> labels(3, 7);
    cusp::permutation_matrix<int, Dev> P;
    cusp::csr_matrix<int, double, Dev> R(3, 4, 0), E(0, 0, 0);
    ASSERT_THROWS(cusp::graph::breadth_first_search(R, 0, labels), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::pseudo_peripheral_vertex(R), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::symmetric_rcm(R, P), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::connected_components(R, labels), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::breadth_first_search(E, 0, labels), cusp::invalid_input_exception);
    ASSERT_EQUAL(cusp::graph::connected_components(E, labels), (size_t)0);
    labels = cusp::array1d<int, Dev>(3, 7);
    const cusp::csr_matrix<int, double, Dev> bad(pattern({{1}, {0, 2}, {1, 9}, {3}}));
    ASSERT_THROWS(cusp::graph::breadth_first_search(bad, 0, labels), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::breadth_first_search(bad, 4, labels), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::breadth_first_search(bad, -1, labels), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::pseudo_peripheral_vertex(bad), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::graph::symmetric_rcm(bad, P), cusp::invalid_input_exception);
    ASSERT_TRUE(cusp::detail::host_copy(labels) == std::vector<int>(3, 7));   // left as it was
    cusp::graph::breadth_first_search(bad, 3, labels);
    ASSERT_TRUE(cusp::detail::host_copy(labels) == std::vector<int>({-1, -1, -1, 0}));
    cusp::permutation_matrix<int, Host> host_wrong(3);
    host_wrong.permutation[1] = 3;
    const cusp::permutation_matrix<int, Dev> wrong(host_wrong), four(4);
    cusp::csr_matrix<int, double, Dev> A(pattern({{0, 1}, {1}, {2}}));
    cusp::array1d<double, Dev> x(3, 1.0), y(3, 0.0), z(4, 0.0);
    ASSERT_THROWS(cusp::multiply(wrong, x, y), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::multiply(x, wrong, y), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::multiply(four, x, y), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::multiply(x, cusp::permutation_matrix<int, Dev>(3), z), cusp::invalid_input_exception);
    ASSERT_THROWS(four.symmetric_permute(A), cusp::invalid_input_exception);
}
DECLARE_UNITTEST(TestRefusals);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }
