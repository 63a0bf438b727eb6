// The named functors through cusp::multiply and cusp::generalized_spmv on device_memory against the host_memory paths of the same program.
// Built and run, in a child process, by tests/test_semiring_gpu.py.
//   (no argument)   the unit tests below
//   decks <file>    every deck of the file (semiring_check.h) on the device, one line per case, after it was compared with the host's bits
//   bellman_ford    `distances <sweeps> <d ...>` of the device run (compared with the host run first)
#include <cmath>
#include <limits>

#include "semiring_check.h"

using namespace semiring_check;
typedef cusp::device_memory Dev;

static const char *const kCombines[] = {"plus", "multiplies", "minimum", "maximum", "project1st", "project2nd"};
static const char *const kReduces[] = {"plus", "multiplies", "minimum", "maximum"};
static const char *const kFormats[] = {"csr", "coo", "ell", "dia", "hyb"};

// poisson5pt nx x ny with values and vectors that hold NaNs, both zeros and infinities; all 24 pairs x 5 formats from y0, from 2.5 and from
// +inf, and through generalized_spmv
template <typename T> deck<T> poisson_deck(size_t nx, size_t ny)
{
    cusp::csr_matrix<int, T, Host> A;
    cusp::gallery::poisson5pt(A, nx, ny);
    deck<T> d;
    d.rows = d.cols = A.num_rows;
    d.nnz = A.num_entries;
    d.width = 3;
    d.offsets = {-(int)nx, -1, 0, 1, (int)nx};
    d.ndiag = 5;
    d.dia_pitch = (d.rows + 31) / 32 * 32;
    d.Ap.assign(A.row_offsets.begin(), A.row_offsets.end());
    d.Aj.assign(A.column_indices.begin(), A.column_indices.end());
    unsigned s = 12345;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return (T)((int)(s >> 16) % 2001 - 1000) / T(256); };
    for (size_t e = 0; e < d.nnz; e++) d.Ax.push_back(next());
    for (size_t j = 0; j < d.cols; j++) d.x.push_back(next());
    for (size_t i = 0; i < d.rows; i++) d.y0.push_back(next());
    const T nan = std::numeric_limits<T>::quiet_NaN(), inf = std::numeric_limits<T>::infinity();
    for (size_t j = 0; j < d.cols; j += 37) d.x[j] = nan;
    for (size_t j = 5; j < d.cols; j += 11) d.x[j] = (j & 1) ? T(0) : -T(0);
    d.x[d.cols / 2] = inf;
    d.y0[3] = -inf;
    d.y0[4] = -T(0);
    for (size_t e = 7; e < d.nnz; e += 13) d.Ax[e] = (e & 1) ? T(0) : -T(0);
    char hex[64];
    std::snprintf(hex, sizeof hex, "%a", 2.5);
    for (const char *c : kCombines)
        for (const char *r : kReduces)
            for (const char *f : kFormats) {
                d.cases.push_back({f, c, r, "y0"});
                d.cases.push_back({f, c, r, hex});
                d.cases.push_back({f, c, r, "inf"});
                d.cases.push_back({std::string("g:") + f, c, r, "y0"});
            }
    return d;
}

template <typename T> void device_equals_host(const deck<T> &d)
{
    const auto want = run_deck<Host>(d);
    const auto got = run_deck<Dev>(d);
    ASSERT_EQUAL(got.size(), want.size());
    for (size_t k = 0; k < got.size(); k++) {
        if (!same_bits(got[k], want[k])) std::printf("  differs: %s %s %s %s\n", d.cases[k].format.c_str(), d.cases[k].combine.c_str(), d.cases[k].reduce.c_str(), d.cases[k].start.c_str());
        ASSERT_TRUE(same_bits(got[k], want[k]));
    }
}

void TestDeviceEqualsHostInEveryFormat()
{
    device_equals_host(poisson_deck<double>(33, 31));
    device_equals_host(poisson_deck<float>(17, 9));
}
DECLARE_UNITTEST(TestDeviceEqualsHostInEveryFormat);

// cusp::hip::par.on(stream) carries the stream through to the semiring kernels
void TestStreamPolicy()
{
    void *stream = nullptr;
    cusp::detail::check(cmi_stream_create(&stream));
    const deck<double> d = poisson_deck<double>(50, 40);
    const cusp::csr_matrix<int, double, Host> H = make_csr(d);
    const cusp::hyb_matrix<int, double, Host> HH = make_hyb(d);
    const cusp::csr_matrix<int, double, Dev> A(H);
    const cusp::hyb_matrix<int, double, Dev> AH(HH);
    const cusp::array1d<double, Host> x(d.x.begin(), d.x.end());
    cusp::array1d<double, Host> y(d.y0.begin(), d.y0.end());
    const cusp::array1d<double, Dev> _x(x);
    cusp::array1d<double, Dev> _y(y), _z(y);
    cusp::multiply(H, x, y, cusp::identity_function<double>(), cusp::plus<double>(), cusp::minimum<double>());
    cusp::multiply(cusp::hip::par.on(stream), A, _x, _y, cusp::identity_function<double>(), cusp::plus<double>(), cusp::minimum<double>());
    cusp::multiply(cusp::hip::par.on(stream), AH, _x, _z, cusp::identity_function<double>(), cusp::plus<double>(), cusp::minimum<double>());
    cusp::detail::check(cmi_stream_synchronize(stream));
    ASSERT_TRUE(same_bits(cusp::detail::host_copy(_y), cusp::detail::host_copy(y)));
    ASSERT_TRUE(same_bits(cusp::detail::host_copy(_z), cusp::detail::host_copy(y)));
    cusp::detail::check(cmi_stream_destroy(stream));
}
DECLARE_UNITTEST(TestStreamPolicy);

// a functor type the library does not know still throws, in every position; nothing falls back to the host
void TestUserFunctorsStillThrow()
{
    cusp::csr_matrix<int, double, Dev> A;
    cusp::gallery::poisson5pt(A, 3, 3);
    cusp::array1d<double, Dev> x(9, 1.0), y(9, 0.0), z(9, 0.0);
    struct maxf { double operator()(double a, double b) const { return a > b ? a : b; } };
    struct twice { double operator()(double a) const { return 2 * a; } };
    ASSERT_THROWS(cusp::multiply(A, x, y, cusp::identity_function<double>(), cusp::plus<double>(), maxf()), cusp::not_implemented_exception);
    ASSERT_THROWS(cusp::multiply(A, x, y, cusp::identity_function<double>(), maxf(), cusp::minimum<double>()), cusp::not_implemented_exception);
    ASSERT_THROWS(cusp::multiply(A, x, y, twice(), cusp::plus<double>(), cusp::minimum<double>()), cusp::not_implemented_exception);
    ASSERT_THROWS(cusp::multiply(A, x, y, cusp::identity_function<double>(), cusp::plus<double>(), cusp::project2nd<double>()), cusp::not_implemented_exception);
    ASSERT_THROWS(cusp::generalized_spmv(A, x, y, z, cusp::plus<double>(), maxf()), cusp::not_implemented_exception);
}
DECLARE_UNITTEST(TestUserFunctorsStillThrow);

// COO entries that are not sorted by row: refused, naming sort_by_row(); after sort_by_row() (stable) the host chains of the unsorted matrix
void TestUnsortedCooThrowsAndWorksAfterSorting()
{
    const deck<double> d = poisson_deck<double>(12, 7);
    cusp::coo_matrix<int, double, Host> H = make_coo(d);
    const size_t n = H.num_entries;
    for (size_t e = 0; e + 1 < n; e += 2) { // swap neighbours, then reverse: rows out of order, and the entries inside a row as well
        std::swap(H.row_indices[e], H.row_indices[e + 1]);
        std::swap(H.column_indices[e], H.column_indices[e + 1]);
        std::swap(H.values[e], H.values[e + 1]);
    }
    for (size_t e = 0; e < n / 2; e++) {
        std::swap(H.row_indices[e], H.row_indices[n - 1 - e]);
        std::swap(H.column_indices[e], H.column_indices[n - 1 - e]);
        std::swap(H.values[e], H.values[n - 1 - e]);
    }
    cusp::coo_matrix<int, double, Dev> A(H);
    const cusp::array1d<double, Host> x(d.x.begin(), d.x.end());
    cusp::array1d<double, Host> y(d.y0.begin(), d.y0.end());
    const cusp::array1d<double, Dev> _x(x);
    cusp::array1d<double, Dev> _y(y);
    bool named = false;
    try { cusp::multiply(A, _x, _y, cusp::identity_function<double>(), cusp::project2nd<double>(), cusp::minimum<double>()); }
    catch (const cusp::not_implemented_exception &e) { named = std::string(e.what()).find("sort_by_row()") != std::string::npos; }
    ASSERT_TRUE(named);
    ASSERT_TRUE(same_bits(cusp::detail::host_copy(_y), cusp::detail::host_copy(y))); // nothing written
    A.sort_by_row();
    cusp::multiply(H, x, y, cusp::identity_function<double>(), cusp::project2nd<double>(), cusp::minimum<double>());
    cusp::multiply(A, _x, _y, cusp::identity_function<double>(), cusp::project2nd<double>(), cusp::minimum<double>());
    ASSERT_TRUE(same_bits(cusp::detail::host_copy(_y), cusp::detail::host_copy(y)));
}
DECLARE_UNITTEST(TestUnsortedCooThrowsAndWorksAfterSorting);

// (constant 0 | identity, multiplies, plus) is the plain multiply's route, bit for bit; a constant other than zero takes the semiring kernel
void TestTheArithmeticPairKeepsItsRoute()
{
    const deck<double> d = poisson_deck<double>(40, 30);
    const cusp::csr_matrix<int, double, Host> H = make_csr(d);
    const cusp::csr_matrix<int, double, Dev> A(H);
    std::vector<double> finite(d.x);
    for (auto &v : finite) if (!(std::fabs(v) < 1e300)) v = 0.5;
    const cusp::array1d<double, Host> x(finite.begin(), finite.end());
    const cusp::array1d<double, Dev> _x(x);
    cusp::array1d<double, Dev> plain(d.rows, 7.0), functors(d.rows, 7.0);
    cusp::multiply(A, _x, plain);
    cusp::multiply(A, _x, functors, cusp::constant_functor<double>(0.0), cusp::multiplies<double>(), cusp::plus<double>());
    ASSERT_TRUE(same_bits(cusp::detail::host_copy(functors), cusp::detail::host_copy(plain)));
    cusp::array1d<double, Host> y(d.rows, 7.0);
    cusp::multiply(H, x, y, cusp::constant_functor<double>(2.5), cusp::multiplies<double>(), cusp::plus<double>());
    cusp::multiply(A, _x, functors, cusp::constant_functor<double>(2.5), cusp::multiplies<double>(), cusp::plus<double>());
    ASSERT_TRUE(same_bits(cusp::detail::host_copy(functors), cusp::detail::host_copy(y)));
}
DECLARE_UNITTEST(TestTheArithmeticPairKeepsItsRoute);

// Bellman-Ford from node 0 on poisson5pt nx x ny with weights |values| (4 on the diagonal, 1 beside it: every sum is exact): one sweep is
// d = min(d, min_j (w_ij + d_j)) -- (plus, minimum) with y0 = y -- until nothing changes
template <typename Space> std::vector<double> bellman_ford(size_t nx, size_t ny, size_t *sweeps)
{
    cusp::csr_matrix<int, double, Host> H;
    cusp::gallery::poisson5pt(H, nx, ny);
    for (size_t e = 0; e < H.num_entries; e++) H.values[e] = std::fabs(H.values[e]);
    const cusp::csr_matrix<int, double, Space> A(H);
    const size_t N = H.num_rows;
    cusp::array1d<double, Host> start(N, std::numeric_limits<double>::infinity());
    start[0] = 0.0;
    cusp::array1d<double, Space> d(start), before(N);
    for (*sweeps = 0; *sweeps <= N;) {
        before = d;
        cusp::multiply(A, before, d, cusp::identity_function<double>(), cusp::plus<double>(), cusp::minimum<double>());
        ++*sweeps;
        if (same_bits(cusp::detail::host_copy(d), cusp::detail::host_copy(before))) break;
    }
    return cusp::detail::host_copy(d);
}

void TestBellmanFordStopsAndEqualsTheHostRun()
{
    size_t hs = 0, ds = 0;
    const std::vector<double> h = bellman_ford<Host>(33, 31, &hs), d = bellman_ford<Dev>(33, 31, &ds);
    ASSERT_TRUE(ds <= 33 * 31 && ds == hs);
    ASSERT_TRUE(same_bits(d, h));
    ASSERT_EQUAL(d[33 * 31 - 1], 32.0 + 30.0);
}
DECLARE_UNITTEST(TestBellmanFordStopsAndEqualsTheHostRun);

template <typename T> int run_decks(std::istream &in)
{
    deck<T> d;
    read_deck(in, d);
    if (!in) return 2;
    const auto want = run_deck<Host>(d);
    const auto got = run_deck<Dev>(d);
    for (size_t k = 0; k < got.size(); k++) {
        if (!same_bits(got[k], want[k])) {
            std::fprintf(stderr, "device differs from host: case %zu (%s %s %s %s)\n", k, d.cases[k].format.c_str(), d.cases[k].combine.c_str(), d.cases[k].reduce.c_str(),
                         d.cases[k].start.c_str());
            return 3;
        }
        print_line(got[k]);
    }
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
    if (argc > 1 && std::string(argv[1]) == "bellman_ford") {
        size_t hs = 0, ds = 0;
        const std::vector<double> h = bellman_ford<Host>(33, 31, &hs), d = bellman_ford<Dev>(33, 31, &ds);
        if (hs != ds || !same_bits(d, h)) return 3;
        std::printf("distances %zu ", ds);
        print_line(d);
        return 0;
    }
    return unittest::run_all(argc, argv);
}
