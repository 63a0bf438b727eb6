// cusp::minimum / maximum / project1st / project2nd and the functor overloads of cusp::multiply and cusp::generalized_spmv on host_memory.
// Built (plain and under AddressSanitizer + UndefinedBehaviorSanitizer) and run by tests/test_semiring_host.py.
//   (no argument)   the unit tests below
//   decks <file>    every deck of the file (semiring_check.h), one line of hexadecimal floats per case
#include <cmath>
#include <limits>

#include "semiring_check.h"

using namespace semiring_check;

// the definitions, ties and NaNs included: not fmin / fmax
void TestNamedFunctorsFollowTheirDefinitions()
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const cusp::minimum<double> lo;
    const cusp::maximum<double> hi;
    ASSERT_TRUE(std::isnan(lo(1.0, nan)) && lo(nan, 1.0) == 1.0);      // a < b ? a : b
    ASSERT_TRUE(hi(1.0, nan) == 1.0 && std::isnan(hi(nan, 1.0)));      // a < b ? b : a
    ASSERT_TRUE(lo(lo(1.0, nan), 2.0) == 2.0 && lo(1.0, lo(nan, 2.0)) == 1.0);
    ASSERT_TRUE(std::signbit(lo(0.0, -0.0)) && !std::signbit(lo(-0.0, 0.0)));   // a tie keeps the second argument
    ASSERT_TRUE(!std::signbit(hi(0.0, -0.0)) && std::signbit(hi(-0.0, 0.0)));   // ... and here the first
    ASSERT_EQUAL(cusp::project1st<float>()(3.0f, 4.0f), 3.0f);
    ASSERT_EQUAL(cusp::project2nd<float>()(3.0f, 4.0f), 4.0f);
}
DECLARE_UNITTEST(TestNamedFunctorsFollowTheirDefinitions);

// min-plus on a path graph: one sweep of Bellman-Ford per call, the distances after n sweeps
void TestMinPlusSweepsOnAPath()
{
    const size_t n = 6;
    cusp::csr_matrix<int, double, Host> A(n, n, 2 * (n - 1));
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        A.row_offsets[i] = (int)at;
        if (i > 0) { A.column_indices[at] = (int)i - 1; A.values[at++] = 2.0; }
        if (i + 1 < n) { A.column_indices[at] = (int)i + 1; A.values[at++] = 3.0; }
    }
    A.row_offsets[n] = (int)at;
    cusp::array1d<double, Host> d(n, std::numeric_limits<double>::infinity());
    d[0] = 0.0;
    for (size_t s = 0; s < n; s++) {
        const cusp::array1d<double, Host> before(d);
        cusp::generalized_spmv(A, before, before, d, cusp::plus<double>(), cusp::minimum<double>());
    }
    for (size_t i = 0; i < n; i++) ASSERT_EQUAL(d[i], 2.0 * (double)i);
}
DECLARE_UNITTEST(TestMinPlusSweepsOnAPath);

// a row maximum of |values| needs no x: project1st; a row without entries keeps the constant
void TestProjectionsAndEmptyRows()
{
    cusp::coo_matrix<int, float, Host> A(4, 3, 3);
    const int I[] = {0, 0, 3}, J[] = {2, 0, 1};
    const float V[] = {-5.0f, 7.0f, 2.0f};
    for (int e = 0; e < 3; e++) { A.row_indices[e] = I[e]; A.column_indices[e] = J[e]; A.values[e] = V[e]; }
    cusp::array1d<float, Host> x(3, 100.0f), y(4, 0.0f);
    cusp::multiply(A, x, y, cusp::constant_functor<float>(-1.0f), cusp::project1st<float>(), cusp::maximum<float>());
    ASSERT_EQUAL(y[0], 7.0f); ASSERT_EQUAL(y[1], -1.0f); ASSERT_EQUAL(y[2], -1.0f); ASSERT_EQUAL(y[3], 2.0f);
    x[0] = 1.0f; x[1] = 2.0f; x[2] = 3.0f;
    cusp::multiply(A, x, y, cusp::identity_function<float>(), cusp::project2nd<float>(), cusp::plus<float>());
    ASSERT_EQUAL(y[0], 11.0f); ASSERT_EQUAL(y[1], -1.0f); ASSERT_EQUAL(y[3], 4.0f);
}
DECLARE_UNITTEST(TestProjectionsAndEmptyRows);

template <typename T> int run_decks(std::istream &in)
{
    deck<T> d;
    read_deck(in, d);
    if (!in) return 2;
    for (const auto &y : run_deck<Host>(d)) print_line(y);
    return 0;
}

int main(int argc, char **argv)
{
    if (argc > 2 && std::string(argv[1]) == "decks") {
        std::ifstream in(argv[2]);
        std::string type;
        while (in >> type) {
            const int st = type == "f64" ? run_decks<double>(in) : run_decks<float>(in);
            if (st) return st;
        }
        return 0;
    }
    return unittest::run_all(argc, argv);
}
