// Shared by the Lanczos test programs (TEST_SPACE / TEST_SPACE_NAME are defined by the including program): cusp::eigen::lanczos, cusp::blas::gemm
// and cusp::detail::tridiagonal_eigen through the real headers in TEST_SPACE.  Modes:
//   (no argument)   the unit tests below: the identity (restarts, beta stored as 0), diag(-5, 2), N = 0 and a wanted count of 0, a wanted count
//                   above N, a restart vector of norm 0 (N = 1), minIter = 1 with three wanted values, a row-major eigVecs, growth of V against a
//                   run that never grows, the three overloads, gemm's shape refusals.
//   "cases"         one line per solver case of tests/lanczos_refs.py CASES (CSR), then 16 x 12 (LA, 4) in the other four formats and through
//                   a matrix-free linear_operator: iterations, converged, the values and the vectors as %a.  On device_memory only the
//                   16 x 12 and 33 x 31 grids, each run fused and with $CMI_LANCZOS_FUSED=0.  The Python side asserts.
//   "gemm FILE"     per line `type m n k lda ldb ldc`, then the values of A (lda x k), B (ldb x n) and C (ldc x n) as %a: cusp::blas::gemm on
//                   views with those pitches; prints all of C afterwards.
//   "tridiag FILE"  per line n, the diagonal, the off-diagonal: prints ok, the eigenvalues and Z (column-major) as %a.
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <cusp/array2d.h>
#include <cusp/coo_matrix.h>
#include <cusp/copy.h>
#include <cusp/csr_matrix.h>
#include <cusp/dia_matrix.h>
#include <cusp/eigen/lanczos.h>
#include <cusp/ell_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/hyb_matrix.h>
#include <cusp/linear_operator.h>

#include "unittest.h"

namespace lanczos_check {

using cusp::eigen::BE;
using cusp::eigen::LA;
using cusp::eigen::SA;
template <typename V> using hcsr = cusp::csr_matrix<int, V, cusp::host_memory>;
template <typename V> using hvec = cusp::array1d<V, cusp::host_memory>;
template <typename V, typename Space> using colmat = cusp::array2d<V, Space, cusp::column_major>;
const bool kDevice = std::strcmp(TEST_SPACE_NAME, "device_memory") == 0;

template <typename V> hcsr<V> poisson(size_t m, size_t n)
{
    hcsr<V> A;
    cusp::gallery::poisson5pt(A, m, n);
    return A;
}
template <typename V> hcsr<V> diagonal_matrix(const std::vector<V> &d)
{
    hcsr<V> A(d.size(), d.size(), d.size());
    for (size_t i = 0; i < d.size(); i++) {
        A.row_offsets[i] = (int)i;
        A.column_indices[i] = (int)i;
        A.values[i] = d[i];
    }
    A.row_offsets[d.size()] = (int)d.size();
    return A;
}

template <typename V> struct solved {
    hvec<V> values;
    colmat<V, cusp::host_memory> vectors;
    cusp::eigen::detail::lanczos_detail::run_info info;
};
template <typename Operator, typename V> solved<V> solve(const Operator &A, size_t wanted, cusp::eigen::lanczos_options<V> options)
{
    cusp::array1d<V, TEST_SPACE> values(wanted, V(-77));
    colmat<V, TEST_SPACE> vectors;
    cusp::eigen::lanczos(A, values, vectors, options);
    solved<V> out;
    out.values = values;
    out.vectors = vectors;
    out.info = cusp::eigen::detail::lanczos_detail::last_run();
    return out;
}
template <typename V> cusp::eigen::lanczos_options<V> full_options(cusp::eigen::SpectrumPart part, double tol)
{
    cusp::eigen::lanczos_options<V> o;
    o.computeEigVecs = true;
    o.reorth = cusp::eigen::Full;
    o.eigPart = part;
    o.tol = V(tol);
    return o;
}

// the identity: every step breaks down, every new vector comes from a restart; T = I
template <typename Space> void TestIdentityRestarts()
{
    const cusp::csr_matrix<int, double, Space> A(diagonal_matrix<double>(std::vector<double>(6, 1.0)));
    const solved<double> s = solve(A, 2, full_options<double>(LA, 1e-10));
    ASSERT_EQUAL(s.values.size(), (size_t)2);
    ASSERT_TRUE(std::abs(s.values[0] - 1.0) <= 1e-14 && std::abs(s.values[1] - 1.0) <= 1e-14);
    ASSERT_TRUE(s.info.restarts >= 1);
    ASSERT_EQUAL(s.vectors.num_rows, (size_t)6);
    ASSERT_EQUAL(s.vectors.num_cols, (size_t)2);
    double dot = 0, n0 = 0, n1 = 0;
    for (size_t i = 0; i < 6; i++) {
        dot += s.vectors(i, 0) * s.vectors(i, 1);
        n0 += s.vectors(i, 0) * s.vectors(i, 0);
        n1 += s.vectors(i, 1) * s.vectors(i, 1);
    }
    ASSERT_TRUE(std::abs(dot) <= 1e-14 && std::abs(n0 - 1) <= 1e-14 && std::abs(n1 - 1) <= 1e-14);
}

template <typename Space> void TestDiagonalTwoByTwo()
{
    const cusp::csr_matrix<int, double, Space> A(diagonal_matrix<double>({-5.0, 2.0}));
    const solved<double> la = solve(A, 1, full_options<double>(LA, 1e-10)), sa = solve(A, 1, full_options<double>(SA, 1e-10)), be = solve(A, 2, full_options<double>(BE, 1e-10));
    ASSERT_TRUE(la.values.size() == 1 && std::abs(la.values[0] - 2.0) <= 1e-14);
    ASSERT_TRUE(sa.values.size() == 1 && std::abs(sa.values[0] + 5.0) <= 1e-14);
    ASSERT_TRUE(be.values.size() == 2 && std::abs(be.values[0] + 5.0) <= 1e-14 && std::abs(be.values[1] - 2.0) <= 1e-14);
    ASSERT_TRUE(std::abs(std::abs(la.vectors(1, 0)) - 1.0) <= 1e-14 && std::abs(la.vectors(0, 0)) <= 1e-14);
}

template <typename Space> void TestEmptyProblems()
{
    const cusp::csr_matrix<int, float, Space> none(hcsr<float>(0, 0, 0)), A(poisson<float>(3, 2));
    solved<float> s = solve(none, 3, full_options<float>(LA, 1e-6));
    ASSERT_TRUE(s.values.size() == 0 && s.vectors.num_cols == 0 && s.info.iterations == 0);
    s = solve(A, 0, full_options<float>(SA, 1e-6));
    ASSERT_TRUE(s.values.size() == 0 && s.vectors.num_cols == 0);
}

// a restart vector whose norm is exactly 0 ends the loop with that step: a 1 x 1 operator through every overload (default options: no
// reorthogonalisation), and diag(-5, 2) without reorthogonalisation, whose two stored vectors span the space
template <typename Space> void TestSpaceExhausted()
{
    const cusp::csr_matrix<int, double, Space> A(diagonal_matrix<double>({3.5}));
    cusp::array1d<double, Space> values(1, -77.0);
    cusp::eigen::lanczos(A, values);
    ASSERT_TRUE(values.size() == 1 && (double)hvec<double>(values)[0] == 3.5);
    // (one step, or two when the normalised start is an ulp off 1 and the first residual is rounding noise instead of 0)
    ASSERT_TRUE(cusp::eigen::detail::lanczos_detail::last_run().iterations <= 2 && cusp::eigen::detail::lanczos_detail::last_run().restarts == 1);
    cusp::array1d<float, Space> three(3, -77.0f);
    colmat<float, Space> E(1, 3);
    const cusp::csr_matrix<int, float, Space> F(diagonal_matrix<float>({-2.0f}));
    cusp::eigen::lanczos(F, three, E);
    ASSERT_TRUE(three.size() == 1 && (float)hvec<float>(three)[0] == -2.0f && E.num_rows == 1 && E.num_cols == 1);
    ASSERT_TRUE(std::abs(colmat<float, cusp::host_memory>(E)(0, 0)) == 1.0f);
    const cusp::csr_matrix<int, double, Space> D(diagonal_matrix<double>({-5.0, 2.0}));
    cusp::eigen::lanczos_options<double> o = full_options<double>(BE, 1e-10);
    o.reorth = cusp::eigen::None;
    const solved<double> s = solve(D, 2, o);
    ASSERT_TRUE(s.values.size() == 2 && std::abs(s.values[0] + 5.0) <= 1e-14 && std::abs(s.values[1] - 2.0) <= 1e-14);
    ASSERT_TRUE(s.info.iterations >= 2 && std::isfinite(s.vectors(0, 0)) && std::isfinite(s.vectors(1, 1))); // (rounding noise decides how many steps)
}

// nine values wanted of a 6 x 6 matrix: six come back, ascending
template <typename Space> void TestWantedCountIsClipped()
{
    const cusp::csr_matrix<int, double, Space> A(poisson<double>(3, 2));
    for (int mode = 0; mode < 2; mode++) {
        cusp::eigen::lanczos_options<double> o = full_options<double>(SA, 1e-10);
        if (mode) o.reorth = cusp::eigen::None;
        const solved<double> s = solve(A, 9, o);
        ASSERT_TRUE(s.values.size() <= 6 && s.vectors.num_cols == s.values.size());
        if (!mode) ASSERT_EQUAL(s.values.size(), (size_t)6);
        for (size_t i = 0; i + 1 < s.values.size(); i++) ASSERT_TRUE(s.values[i] <= s.values[i + 1]);
    }
}

// a first check at step 1 with three values wanted: T_0 and T_1 have fewer values than the sums would read
template <typename Space> void TestMinIterOne()
{
    const cusp::csr_matrix<int, double, Space> A(poisson<double>(7, 5));
    for (int part = 0; part < 3; part++) {
        cusp::eigen::lanczos_options<double> o = full_options<double>(part == 0 ? SA : (part == 1 ? LA : BE), 1e-10);
        o.minIter = 1;
        o.stride = 1;
        const solved<double> s = solve(A, 3, o);
        ASSERT_EQUAL(s.values.size(), (size_t)3);
        ASSERT_TRUE(s.info.iterations >= 3 && s.info.iterations <= 35);
    }
}

template <typename Space> void TestRowMajorIsRefused()
{
    const cusp::csr_matrix<int, double, Space> A(poisson<double>(3, 2)), R(hcsr<double>(5, 6, 0));
    cusp::array1d<double, Space> values(2);
    cusp::array2d<double, Space, cusp::row_major> rows;
    colmat<double, Space> cols;
    cusp::eigen::lanczos_options<double> o = full_options<double>(LA, 1e-10);
    ASSERT_THROWS(cusp::eigen::lanczos(A, values, rows, o), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::eigen::lanczos(R, values, cols, o), cusp::invalid_input_exception);
}

// V grown from three columns by the factor 1.2 against V allocated once: the same bits (16 x 12, 30 steps: no test converges that early)
template <typename V, typename Space> void growth_case(cusp::eigen::ReorthStrategy reorth)
{
    const cusp::csr_matrix<int, V, Space> A(poisson<V>(16, 12));
    cusp::eigen::lanczos_options<V> grown = full_options<V>(BE, std::is_same<V, double>::value ? 1e-10 : 1e-6), fixed = grown;
    grown.reorth = fixed.reorth = reorth;
    grown.maxIter = fixed.maxIter = 30;
    grown.minIter = 3;
    fixed.minIter = 30;
    const solved<V> a = solve(A, 5, grown), b = solve(A, 5, fixed);
    ASSERT_TRUE(a.info.iterations == 30 && b.info.iterations == 30 && !a.info.converged && !b.info.converged);
    ASSERT_EQUAL(a.values.size(), (size_t)5);
    ASSERT_TRUE(std::memcmp(a.values.data(), b.values.data(), 5 * sizeof(V)) == 0);
    ASSERT_EQUAL(a.vectors.values.size(), b.vectors.values.size());
    ASSERT_TRUE(std::memcmp(a.vectors.values.data(), b.vectors.values.data(), a.vectors.values.size() * sizeof(V)) == 0);
}
template <typename Space> void TestGrowthChangesNothing()
{
    growth_case<double, Space>(cusp::eigen::Full);
    growth_case<float, Space>(cusp::eigen::Full);
    growth_case<double, Space>(cusp::eigen::None);
}

// lanczos(A, eigVals) and lanczos(A, eigVals, eigVecs): default options (LA, no reorthogonalisation, tol 1e-4); vectors when eigVecs has columns
template <typename Space> void TestOverloads()
{
    const cusp::csr_matrix<int, double, Space> A(poisson<double>(16, 12));
    const double pi = 3.14159265358979323846, top = 4 + 2 * std::cos(pi / 17) + 2 * std::cos(pi / 13);
    cusp::array1d<double, Space> one(1), two(1);
    cusp::eigen::lanczos(A, one);
    ASSERT_TRUE(std::abs((double)hvec<double>(one)[0] - top) <= 1e-3);
    colmat<double, Space> E(192, 1);
    cusp::eigen::lanczos(A, two, E);
    ASSERT_TRUE(std::abs((double)hvec<double>(two)[0] - top) <= 1e-3 && E.num_rows == 192 && E.num_cols == 1);
    colmat<double, Space> none;
    cusp::eigen::lanczos(A, two, none);
    ASSERT_EQUAL(none.num_cols, (size_t)0);
}

template <typename Space> void TestGemmShapes()
{
    colmat<float, Space> A(5, 3, 1.0f), B(3, 2, 2.0f), C(5, 2, -1.0f), B4(4, 2, 1.0f), C3(5, 3, 0.0f), C6(6, 2, 0.0f);
    cusp::blas::gemm(A, B, C);
    const colmat<float, cusp::host_memory> h(C);
    for (size_t i = 0; i < 5; i++)
        for (size_t j = 0; j < 2; j++) ASSERT_TRUE(h(i, j) == 6.0f);
    ASSERT_THROWS(cusp::blas::gemm(A, B4, C), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::blas::gemm(A, B, C3), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::blas::gemm(A, B, C6), cusp::invalid_input_exception);
    colmat<float, Space> A0(5, 0), B0(0, 2); // k == 0: +0 everywhere
    cusp::blas::gemm(A0, B0, C);
    const colmat<float, cusp::host_memory> z(C);
    for (size_t i = 0; i < 10; i++) ASSERT_TRUE(z.values[i] == 0.0f && !std::signbit(z.values[i]));
}

// ---- "cases" ---------------------------------------------------------------------------------------------------------------------------------
template <typename V, typename Space> struct wrapped_operator : cusp::linear_operator<V, Space> {
    cusp::csr_matrix<int, V, Space> A;
    explicit wrapped_operator(const hcsr<V> &H) : cusp::linear_operator<V, Space>(H.num_rows, H.num_cols, H.num_entries), A(H) {}
    template <typename X, typename Y> void operator()(const X &x, Y &y) const { cusp::multiply(A, x, y); }
};

inline cusp::eigen::SpectrumPart part_of(const char *name) { return std::strcmp(name, "SA") == 0 ? SA : (std::strcmp(name, "LA") == 0 ? LA : BE); }

template <typename Operator, typename V>
void print_runs(const Operator &A, size_t nx, size_t ny, const char *type, const char *part, size_t count, const char *reorth, double tol, const char *format)
{
    const char *runs[2] = {"fused", "plain"};
    for (int r = 0; r < (kDevice ? 2 : 1); r++) {
        if (kDevice) setenv("CMI_LANCZOS_FUSED", r == 1 ? "0" : "1", 1);
        cusp::eigen::lanczos_options<V> o = full_options<V>(part_of(part), tol);
        if (std::strcmp(reorth, "None") == 0) o.reorth = cusp::eigen::None;
        const solved<V> s = solve(A, count, o);
        std::printf("case %zu %zu %s %s %zu %s %g %s run %s iterations %zu converged %d found %zu rows %zu values", nx, ny, type, part, count, reorth, tol, format,
                    kDevice ? runs[r] : "host", s.info.iterations, (int)s.info.converged, s.values.size(), s.vectors.num_rows);
        for (size_t i = 0; i < s.values.size(); i++) std::printf(" %a", (double)s.values[i]);
        std::printf(" vectors");
        for (size_t j = 0; j < s.vectors.num_cols; j++)
            for (size_t i = 0; i < s.vectors.num_rows; i++) std::printf(" %a", (double)s.vectors(i, j));
        std::printf("\n");
    }
    if (kDevice) unsetenv("CMI_LANCZOS_FUSED");
}

template <typename V> void print_grid(size_t nx, size_t ny, const char *type, double tol)
{
    typedef TEST_SPACE Space;
    const hcsr<V> H = poisson<V>(nx, ny);
    const cusp::csr_matrix<int, V, Space> A(H);
    const char *parts[4] = {"LA", "LA", "SA", "BE"};
    const size_t counts[4] = {1, 4, 4, 5};
    for (int k = 0; k < 4; k++) print_runs<decltype(A), V>(A, nx, ny, type, parts[k], counts[k], "Full", tol, "csr");
    if (nx != 16) return;
    print_runs<decltype(A), V>(A, nx, ny, type, "LA", 1, "None", tol, "csr");
    print_runs<cusp::coo_matrix<int, V, Space>, V>(cusp::coo_matrix<int, V, Space>(H), nx, ny, type, "LA", 4, "Full", tol, "coo");
    print_runs<cusp::ell_matrix<int, V, Space>, V>(cusp::ell_matrix<int, V, Space>(H), nx, ny, type, "LA", 4, "Full", tol, "ell");
    print_runs<cusp::dia_matrix<int, V, Space>, V>(cusp::dia_matrix<int, V, Space>(H), nx, ny, type, "LA", 4, "Full", tol, "dia");
    print_runs<cusp::hyb_matrix<int, V, Space>, V>(cusp::hyb_matrix<int, V, Space>(H), nx, ny, type, "LA", 4, "Full", tol, "hyb");
    print_runs<wrapped_operator<V, Space>, V>(wrapped_operator<V, Space>(H), nx, ny, type, "LA", 4, "Full", tol, "operator");
}

inline int print_cases()
{
    if (!kDevice) {
        print_grid<double>(7, 5, "f64", 1e-10);
        print_grid<float>(7, 5, "f32", 1e-6);
    }
    print_grid<double>(16, 12, "f64", 1e-10);
    print_grid<float>(16, 12, "f32", 1e-6);
    print_grid<double>(33, 31, "f64", 1e-10);
    return 0;
}

// ---- "gemm FILE" -----------------------------------------------------------------------------------------------------------------------------
template <typename V> bool read_values(std::FILE *f, hvec<V> &a)
{
    for (size_t i = 0; i < a.size(); i++) {
        double v;
        if (std::fscanf(f, "%la", &v) != 1) return false;
        a[i] = static_cast<V>(v);
    }
    return true;
}
template <typename V> int gemm_line(std::FILE *f, size_t m, size_t n, size_t k, size_t lda, size_t ldb, size_t ldc)
{
    hvec<V> a(lda * k), b(ldb * n), c(ldc * n);
    if (!read_values(f, a) || !read_values(f, b) || !read_values(f, c)) return 2;
    cusp::array1d<V, TEST_SPACE> da(a), db(b), dc(c);
    const cusp::array2d_column_view<const V, TEST_SPACE> A(m, k, lda, da.data()), B(k, n, ldb, db.data());
    cusp::array2d_column_view<V, TEST_SPACE> C(m, n, ldc, dc.data());
    cusp::blas::gemm(A, B, C);
    const hvec<V> out(dc), a_after(da), b_after(db);
    if (std::memcmp(a_after.data(), a.data(), a.size() * sizeof(V)) != 0 || std::memcmp(b_after.data(), b.data(), b.size() * sizeof(V)) != 0) return 3;
    for (size_t i = 0; i < out.size(); i++) std::printf("%s%a", i ? " " : "", (double)out[i]);
    std::printf("\n");
    return 0;
}
inline int print_gemm(const char *path)
{
    std::FILE *f = std::fopen(path, "r");
    if (!f) return 2;
    char type[8];
    size_t m, n, k, lda, ldb, ldc;
    int status = 0;
    while (status == 0 && std::fscanf(f, "%7s %zu %zu %zu %zu %zu %zu", type, &m, &n, &k, &lda, &ldb, &ldc) == 7)
        status = std::strcmp(type, "f64") == 0 ? gemm_line<double>(f, m, n, k, lda, ldb, ldc) : gemm_line<float>(f, m, n, k, lda, ldb, ldc);
    std::fclose(f);
    return status;
}

// ---- "tridiag FILE" --------------------------------------------------------------------------------------------------------------------------
inline int print_tridiag(const char *path)
{
    std::FILE *f = std::fopen(path, "r");
    if (!f) return 2;
    size_t n;
    while (std::fscanf(f, "%zu", &n) == 1) {
        std::vector<double> d(n), e(n ? n - 1 : 0), w(n), Z(n * n);
        for (double &v : d) if (std::fscanf(f, "%la", &v) != 1) return 2;
        for (double &v : e) if (std::fscanf(f, "%la", &v) != 1) return 2;
        const bool ok = cusp::detail::tridiagonal_eigen(n, d.data(), e.data(), w.data(), Z.data());
        std::printf("%d", (int)ok);
        for (size_t i = 0; ok && i < n; i++) std::printf(" %a", w[i]);
        for (size_t i = 0; ok && i < n * n; i++) std::printf(" %a", Z[i]);
        std::printf("\n");
        std::vector<double> w2(n); // without vectors: the same values
        if (!cusp::detail::tridiagonal_eigen(n, d.data(), e.data(), w2.data(), nullptr) || (ok && std::memcmp(w.data(), w2.data(), n * sizeof(double)) != 0)) return 3;
    }
    std::fclose(f);
    return 0;
}

} // namespace lanczos_check
