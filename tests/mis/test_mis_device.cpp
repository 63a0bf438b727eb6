// cusp::graph::maximal_independent_set, mis_aggregate and smoothed_aggregation::mis_aggregation on device_memory against the
// host_memory paths of the same program.  Built and run once, in a child process, by tests/test_mis_gpu.py.
#include "mis_check.h"

using namespace mis_check;
typedef cusp::device_memory Dev;
typedef cusp::host_memory Host;

// stencils of MIS(0..3) with their sizes and rounds, aggregates and mis: the five device formats against the host CSR path
void TestDeviceEqualsHostInEveryFormat()
{
    for (auto &g : reference_graphs())
        for (uint64_t seed : {0ull, 0x1234567ull}) {
            const result want = run(g.second, seed);
            if (!five_formats_give<Dev>(g.second, seed, want)) std::printf("  differs: %s, seed %llu\n", g.first.c_str(), (unsigned long long)seed);
            ASSERT_TRUE(five_formats_give<Dev>(g.second, seed, want));
        }
}
DECLARE_UNITTEST(TestDeviceEqualsHostInEveryFormat);

// a pattern that is not symmetric, with isolated nodes, empty rows, repeated columns and rows without a diagonal; the public
// overloads and other stencil types
void TestIrregularPatternAndOverloads()
{
    const host_csr<double> A = irregular_square<double>(1500, 9, 77);
    const cusp::csr_matrix<int, double, Dev> dA(A);
    ASSERT_TRUE(run(dA, 0) == run(A, 0));
    ASSERT_TRUE(run(dA, 5) == run(A, 5));
    const result r = run(A, 0);
    ASSERT_TRUE(std::count(r.aggregates.begin(), r.aggregates.end(), -1) > 0);
    cusp::array1d<int, Dev> stencil;
    cusp::array1d<char, Dev> bytes;
    cusp::array1d<int, Host> on_host;
    const cusp::csr_matrix<int, float, Dev> P(poisson(13, 17));
    ASSERT_EQUAL(cusp::graph::maximal_independent_set(P, stencil), (size_t)88);
    ASSERT_EQUAL(cusp::graph::maximal_independent_set(cusp::hip::par, P, bytes, 2), (size_t)34);
    ASSERT_EQUAL(cusp::graph::maximal_independent_set(P, on_host, 2), (size_t)34);
    ASSERT_TRUE(cusp::detail::host_copy(bytes) == std::vector<char>(on_host.begin(), on_host.end()));
    ASSERT_EQUAL(cusp::graph::maximal_independent_set(P, stencil, 0), (size_t)221);
    ASSERT_TRUE(cusp::detail::host_copy(stencil) == std::vector<int>(221, 1));
    cusp::csr_matrix<int, double, Dev> R(3, 4, 0), E(0, 0, 0);
    ASSERT_THROWS(cusp::graph::maximal_independent_set(R, stencil), cusp::invalid_input_exception);
    ASSERT_EQUAL(cusp::graph::maximal_independent_set(E, stencil, 2), (size_t)0);
    const cusp::csr_matrix<int, double, Dev> bad(pattern({{0, 1}, {0, 2}}));
    ASSERT_THROWS(cusp::graph::maximal_independent_set(bad, stencil), cusp::invalid_input_exception);
}
DECLARE_UNITTEST(TestIrregularPatternAndOverloads);

// the mis_aggregation hierarchy on poisson 100x100 with the HOST's rho per level: aggregates, sizes and entry counts identical,
// every matrix bit for bit (compared the way test_amg_device.cpp compares the standard one)
void TestMisHierarchyEqualsTheHostOne()
{
    const host_csr<double> A = poisson(100, 100);
    agg::smoothed_aggregation<int, double, Host> M;
    M.mis_aggregation = true;
    M.initialize(A);
    std::vector<double> rhos;
    for (size_t i = 0; i + 1 < M.sa_levels.size(); i++) rhos.push_back(M.sa_levels[i].rho_DinvA);
    const std::vector<built_level<double, Host>> H = build_mis<double, Host>(A, rhos, 500);
    const std::vector<built_level<double, Dev>> D = build_mis<double, Dev>(cusp::csr_matrix<int, double, Dev>(A), rhos, 500);
    ASSERT_EQUAL(H.size(), M.levels.size());
    ASSERT_EQUAL(D.size(), H.size());
    ASSERT_EQUAL(H[1].A.num_rows, (size_t)1422);
    for (size_t l = 0; l < H.size(); l++) {
        ASSERT_TRUE(csr_bits_equal(H[l].A, M.levels[l].A));
        ASSERT_TRUE(csr_bits_equal(D[l].A, H[l].A));
        ASSERT_TRUE(arrays_bits_equal(D[l].B, H[l].B));
        if (l + 1 == H.size()) break;
        ASSERT_TRUE(arrays_bits_equal(D[l].aggregates, H[l].aggregates));
        ASSERT_TRUE(csr_bits_equal(D[l].S, H[l].S));
        ASSERT_TRUE(csr_bits_equal(D[l].T, H[l].T));
        ASSERT_TRUE(csr_bits_equal(D[l].P, H[l].P));
        ASSERT_TRUE(csr_bits_equal(D[l].R, H[l].R));
    }
}
DECLARE_UNITTEST(TestMisHierarchyEqualsTheHostOne);

// the class itself on the device: the host class's levels, a working preconditioner, the flag kept by the cross-space copy
void TestClassWithMisAggregation()
{
    const host_csr<double> A = poisson(100, 100);
    const cusp::csr_matrix<int, double, Dev> dA(A);
    agg::smoothed_aggregation<int, double, Host> MH;
    agg::smoothed_aggregation<int, double, Dev> MD;
    MH.mis_aggregation = MD.mis_aggregation = true;
    MH.initialize(A);
    MD.initialize(dA);
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
    std::printf("  cg iterations (10000 rows, MIS(2) aggregation): device preconditioner %ld, host preconditioner %ld, none %ld\n", device_count, host_count, plain);
    ASSERT_TRUE(device_count > 0 && device_count < plain);
    ASSERT_TRUE(device_count <= host_count + 2);
    agg::smoothed_aggregation<int, double, Host> copy(MD);
    ASSERT_TRUE(copy.mis_aggregation);
    ASSERT_TRUE(cg_count(A, hb, &copy) <= host_count + 2);
}
DECLARE_UNITTEST(TestClassWithMisAggregation);

int main(int argc, char **argv) { return unittest::run_all(argc, argv); }
