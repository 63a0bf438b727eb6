// Evolution strength of connection and cusp::gallery::diffusion on host_memory (tests/test_evolution_host.py builds and runs this,
// plainly and under the address and undefined-behaviour sanitizers).  "--measure f64|f32 deck..." prints the measure of decks
// written by the Python side, which compares them with tests/evolution_refs.py bit for bit.
#include "evolution_check.h"

using namespace evolution_check;
namespace gallery = cusp::gallery;

template <typename V> host_csr<V> from_rows(size_t n, const std::vector<std::vector<int>> &rows)
{
    size_t entries = 0;
    for (auto &r : rows) entries += r.size();
    host_csr<V> A(n, n, entries);
    size_t at = 0;
    for (size_t i = 0; i < rows.size(); i++) {
        A.row_offsets[i] = (int)at;
        for (int j : rows[i]) {
            A.column_indices[at] = j;
            A.values[at] = (size_t)j == i ? V(4) : V(-1);
            at++;
        }
    }
    A.row_offsets[rows.size()] = (int)at;
    return A;
}

template <typename V> void TestRefusals()
{
    host_csr<V> S;
    cusp::array1d<V, cusp::host_memory> B3(3, V(1)), B2(2, V(1));
    host_csr<V> rect(2, 3, 0);
    for (size_t i = 0; i <= 2; i++) rect.row_offsets[i] = 0;
    ASSERT_THROWS(agg::evolution_strength_of_connection(rect, S, B2, 1.5), cusp::invalid_input_exception);                                        // not square
    ASSERT_THROWS(agg::evolution_strength_of_connection(from_rows<V>(3, {{0, 1}, {1}, {2}}), S, B3, 1.5), cusp::invalid_input_exception);         // (0,1) without (1,0)
    ASSERT_THROWS(agg::evolution_strength_of_connection(from_rows<V>(3, {{0, 2, 1}, {0, 1}, {0, 2}}), S, B3, 1.5), cusp::invalid_input_exception); // unsorted row
    ASSERT_THROWS(agg::evolution_strength_of_connection(from_rows<V>(2, {{0, 1, 1}, {0, 1}}), S, B2, 1.5), cusp::invalid_input_exception);        // repeated column
    ASSERT_THROWS(agg::evolution_strength_of_connection(from_rows<V>(2, {{0, 2}, {0, 1}}), S, B2, 1.5), cusp::invalid_input_exception);           // column outside
    ASSERT_THROWS(agg::evolution_strength_of_connection(from_rows<V>(2, {{0, 1}, {0, 1}}), S, B3, 1.5), cusp::invalid_input_exception);           // B of another size
    ASSERT_THROWS(agg::evolution_strength_of_connection(from_rows<V>(2, {{0, 1}, {0, 1}}), S, B2, std::nan("")), cusp::invalid_input_exception);  // rho not finite
    agg::evolution_strength_of_connection(from_rows<V>(2, {{0, 1}, {0, 1}}), S, B2, 1.5);
    ASSERT_EQUAL(S.num_rows, (size_t)2);
    host_csr<V> empty(0, 0, 0), kept;
    empty.row_offsets[0] = 0;
    agg::evolution_strength_of_connection(empty, kept, cusp::array1d<V, cusp::host_memory>(), 0.0);
    ASSERT_EQUAL(kept.num_entries, (size_t)0);
}
void TestRefusalsF64() { TestRefusals<double>(); }
void TestRefusalsF32() { TestRefusals<float>(); }
DECLARE_UNITTEST(TestRefusalsF64);
DECLARE_UNITTEST(TestRefusalsF32);

// diffusion into all five formats: the CSR form of each equals the CSR matrix; entry counts of the 7 x 5 grid
template <typename Matrix> void TestDiffusionFormats()
{
    typedef typename Matrix::value_type V;
    for (int fe = 0; fe < 2; fe++)
        for (double angle : {0.0, M_PI / 4}) {
            host_csr<V> want;
            Matrix got;
            if (fe) { gallery::diffusion<gallery::FE>(want, 7, 5, 1e-3, angle); gallery::diffusion<gallery::FE>(got, 7, 5, 1e-3, angle); }
            else { gallery::diffusion<gallery::FD>(want, 7, 5, 1e-3, angle); gallery::diffusion<gallery::FD>(got, 7, 5, 1e-3, angle); }
            ASSERT_EQUAL(want.num_entries, (size_t)((!fe && angle == 0.0) ? 151 : 247)); // FD at angle 0: a and c are exactly zero and leave no entry
            for (size_t e = 0; e < want.num_entries; e++) ASSERT_TRUE(want.values[e] != V(0));
            ASSERT_EQUAL(got.num_rows, (size_t)35);
            ASSERT_TRUE(csr_bits_equal(host_csr<V>(got), want));
        }
    Matrix defaults; // eps = 1e-5, theta = pi / 4
    host_csr<V> want;
    gallery::diffusion<gallery::FE>(defaults, 4, 3);
    gallery::diffusion<gallery::FE>(want, 4, 3, 1e-5, M_PI / 4);
    ASSERT_TRUE(csr_bits_equal(host_csr<V>(defaults), want));
}
#define TEST_SPACE cusp::host_memory
#define TEST_SPACE_NAME "host_memory"
DECLARE_SPARSE_MATRIX_UNITTEST(TestDiffusionFormats);

// the strong direction and nothing else, with rho estimated by the measure itself (step 3)
template <typename V> void TestSevenByFive()
{
    for (int fe = 0; fe < 2; fe++)
        for (double eps : {1e-3, 1e-2}) {
            host_csr<V> A, S;
            if (fe) gallery::diffusion<gallery::FE>(A, 7, 5, eps, 0.0);
            else gallery::diffusion<gallery::FD>(A, 7, 5, eps, 0.0);
            const cusp::array1d<V, cusp::host_memory> B(A.num_rows, V(1));
            agg::evolution_strength_of_connection(A, S, B);
            ASSERT_EQUAL(S.num_entries, (size_t)91);
            ASSERT_TRUE(diagonals_of(S) == (std::set<long>{-7, 0, 7}));
            // COO operands give the same entries; the policy overload is the same call
            cusp::coo_matrix<int, V, cusp::host_memory> Acoo(A), Scoo;
            agg::evolution_strength_of_connection(Acoo, Scoo, B);
            ASSERT_TRUE(csr_bits_equal(host_csr<V>(Scoo), S));
            host_csr<V> S2;
            struct my_policy : cusp::execution_policy<my_policy> {} exec;
            agg::evolution_strength_of_connection(exec, A, S2, B, 0.0, 4.0);
            ASSERT_TRUE(csr_bits_equal(S2, S));
        }
}
void TestSevenByFiveF64() { TestSevenByFive<double>(); }
void TestSevenByFiveF32() { TestSevenByFive<float>(); }
DECLARE_UNITTEST(TestSevenByFiveF64);
DECLARE_UNITTEST(TestSevenByFiveF32);

// diffusion<FD> 40 x 30, eps 1e-3, angle 0, double, levels down to 100 rows, cg to 1e-8.  Measured on host_memory:
//   symmetric strength (theta 0): 91 iterations, levels 1200 / 210 / 25
//   evolution strength:           11 iterations, levels 1200 / 400 / 160 / 80   (with MIS(2) aggregation: 17, levels 1200 / 346 / 113 / 40)
// The condition: both converge and the evolution run takes at most half the iterations of the symmetric run.
void TestSmoothedAggregationOnAnisotropy()
{
    const sa_run symmetric = anisotropic_cg<cusp::host_memory>(false), evolution = anisotropic_cg<cusp::host_memory>(true), with_mis = anisotropic_cg<cusp::host_memory>(true, true);
    print_run("symmetric strength", symmetric);
    print_run("evolution strength", evolution);
    print_run("evolution strength, MIS aggregation", with_mis);
    ASSERT_TRUE(symmetric.iterations > 0 && evolution.iterations > 0 && with_mis.iterations > 0);
    ASSERT_TRUE(2 * evolution.iterations <= symmetric.iterations);
    ASSERT_TRUE(evolution.level_rows.size() >= 3 && evolution.level_rows[1] > symmetric.level_rows[1]); // aggregates along the strong direction only: a slower coarsening
}
DECLARE_UNITTEST(TestSmoothedAggregationOnAnisotropy);

void TestMembersAreCarriedAcrossSpaces()
{
    agg::smoothed_aggregation<int, double, cusp::host_memory> M;
    ASSERT_TRUE(!M.evolution_strength && M.evolution_epsilon == 4.0);
    M.evolution_strength = true;
    M.evolution_epsilon = 2.5;
    host_csr<double> A;
    gallery::diffusion<gallery::FD>(A, 12, 10, 1e-3, 0.0);
    M.min_level_size = 30;
    M.initialize(A);
    ASSERT_TRUE(M.sa_levels.size() >= 2 && M.sa_levels[0].rho_DinvA > 0.0);
    const agg::smoothed_aggregation<int, double, cusp::host_memory> C(M);
    ASSERT_TRUE(C.evolution_strength && C.evolution_epsilon == 2.5 && C.sa_levels.size() == M.sa_levels.size());
}
DECLARE_UNITTEST(TestMembersAreCarriedAcrossSpaces);

int main(int argc, char **argv)
{
    if (argc >= 4 && std::string(argv[1]) == "--measure")
        return std::string(argv[2]) == "f32" ? print_measures<float, cusp::host_memory>(argc, argv) : print_measures<double, cusp::host_memory>(argc, argv);
    return unittest::run_all(argc, argv);
}
