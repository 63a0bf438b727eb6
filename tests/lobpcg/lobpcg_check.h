// Shared by the LOBPCG test programs (TEST_SPACE / TEST_SPACE_NAME are defined by the including program): cusp::eigen::lobpcg through the real
// headers in TEST_SPACE.  Two modes:
//   (no argument)  the unit tests below: all five formats and a matrix-free linear_operator on Poisson 10 x 10 (whose extreme eigenvalues are
//                  known in closed form), X as an array2d, the three overloads, the min(N, limit) cap, the breakdown rule of the Rayleigh-Ritz
//                  step (reached through detail::lobpcg_detail::ritz_step), the shape exceptions.
//   "cases"        one line per solver case of tests/lobpcg_refs.py CASES (CSR; start vector cusp::random_array<T>(N, 7); monitor(ones, 500,
//                  tolerance)): iterations, converged, S[0], ||x||, the true residual ||A x - S[0] x|| recomputed in double.  On device_memory
//                  each case runs three times: fused, fused again, $CMI_LOBPCG_FUSED=0.  The Python side asserts (it has the exact eigenvalues
//                  and the restatement's iteration counts).
#pragma once
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <cusp/array2d.h>
#include <cusp/coo_matrix.h>
#include <cusp/copy.h>
#include <cusp/csr_matrix.h>
#include <cusp/dia_matrix.h>
#include <cusp/eigen/lobpcg.h>
#include <cusp/ell_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/hyb_matrix.h>
#include <cusp/precond/diagonal.h>

#include "unittest.h"

namespace lobpcg_check {

template <typename V> using hcsr = cusp::csr_matrix<int, V, cusp::host_memory>;
template <typename V> using hvec = cusp::array1d<V, cusp::host_memory>;
template <typename V> struct bars;
template <> struct bars<float> { static constexpr double tolerance = 1e-3; };
template <> struct bars<double> { static constexpr double tolerance = 1e-8; };
const size_t kLimit = 500;
const double kPi = 3.14159265358979323846;

template <typename V> hcsr<V> poisson(size_t m, size_t n)
{
    hcsr<V> A;
    cusp::gallery::poisson5pt(A, m, n);
    return A;
}
// A_1 = poisson5pt + diag(1 + i mod 7)
template <typename V> hcsr<V> poisson_plus_diagonal(size_t m, size_t n)
{
    hcsr<V> A = poisson<V>(m, n);
    for (size_t i = 0; i < A.num_rows; i++)
        for (int jj = A.row_offsets[i]; jj < A.row_offsets[i + 1]; jj++)
            if ((size_t)A.column_indices[jj] == i) A.values[jj] = A.values[jj] + V(1 + i % 7);
    return A;
}
// the extreme eigenvalues of poisson5pt(m, n): 4 -+ 2 cos(pi / (m + 1)) -+ 2 cos(pi / (n + 1))
inline double poisson_eigenvalue(size_t m, size_t n, bool largest)
{
    const double c = 2 * std::cos(kPi / (m + 1)) + 2 * std::cos(kPi / (n + 1));
    return largest ? 4 + c : 4 - c;
}

struct outcome { size_t iterations; bool converged; double lambda, x_norm, residual; };

// ||x|| and ||A x - lambda x|| in double on the host, whatever space the solve ran in
template <typename V> void measure(const hcsr<V> &H, const hvec<V> &x, double lambda, outcome &o)
{
    double xx = 0, rr = 0;
    for (size_t i = 0; i < H.num_rows; i++) {
        double acc = -lambda * (double)x[i];
        for (int jj = H.row_offsets[i]; jj < H.row_offsets[i + 1]; jj++) acc += (double)H.values[jj] * (double)x[H.column_indices[jj]];
        rr += acc * acc;
        xx += (double)x[i] * (double)x[i];
    }
    o.x_norm = std::sqrt(xx);
    o.residual = std::sqrt(rr);
}

template <typename V> cusp::array1d<V, TEST_SPACE> start_vector(size_t N)
{
    cusp::array1d<V, TEST_SPACE> x(N);
    cusp::copy(cusp::random_array<V>(N, 7), x);
    return x;
}

// one solve: Matrix over TEST_SPACE built from H; with_diagonal: M = cusp::precond::diagonal, else the four-argument overload
template <typename Matrix> outcome solve(const hcsr<typename Matrix::value_type> &H, double tolerance, bool largest, bool with_diagonal, size_t limit = kLimit)
{
    typedef typename Matrix::value_type V;
    const Matrix A(H);
    const size_t N = A.num_rows;
    cusp::array1d<V, TEST_SPACE> S(1, V(0)), X = start_vector<V>(N);
    const hvec<V> ones(N, V(1));
    cusp::monitor<V> monitor(ones, limit, V(tolerance));
    if (with_diagonal) {
        cusp::precond::diagonal<V, TEST_SPACE> M(A);
        cusp::eigen::lobpcg(A, S, X, monitor, M, largest);
    } else {
        cusp::eigen::lobpcg(A, S, X, monitor, largest);
    }
    outcome o = {monitor.iteration_count(), monitor.converged(), (double)hvec<V>(S)[0], 0, 0};
    measure(H, hvec<V>(X), o.lambda, o);
    return o;
}

inline void expect(bool ok, const std::string &what, const outcome &o, double want)
{
    if (ok) return;
    char msg[384];
    std::snprintf(msg, sizeof msg, "%s in %s: iterations %zu, converged %d, lambda %.17g (want %.17g), | ||x|| - 1 | %.3g, residual %.3g", what.c_str(), TEST_SPACE_NAME,
                  o.iterations, (int)o.converged, o.lambda, want, std::abs(o.x_norm - 1), o.residual);
    throw unittest::failure(msg);
}
inline void check_outcome(const outcome &o, double want, double tolerance, size_t N, const std::string &what)
{
    expect(o.converged, what + ": not converged", o, want);
    expect(std::abs(o.lambda - want) <= tolerance, what + ": eigenvalue", o, want);
    expect(o.residual <= 2 * tolerance, what + ": true residual", o, want);
    expect(std::abs(o.x_norm - 1) <= 1e-5, what + ": norm of x", o, want);
    expect(o.iterations <= std::min(N, kLimit), what + ": iteration count", o, want);
}

// all five formats x float, double on Poisson 10 x 10: the smallest eigenvalue, and the largest in double
template <typename Matrix> void TestFormats()
{
    typedef typename Matrix::value_type V;
    const hcsr<V> H = poisson<V>(10, 10);
    check_outcome(solve<Matrix>(H, bars<V>::tolerance, false, false), poisson_eigenvalue(10, 10, false), bars<V>::tolerance, 100, "poisson10x10 smallest");
    if (std::is_same<V, double>::value)
        check_outcome(solve<Matrix>(H, bars<V>::tolerance, true, false), poisson_eigenvalue(10, 10, true), bars<V>::tolerance, 100, "poisson10x10 largest");
}

// a matrix-free operator: y <- A x through a CSR it holds, with no format of its own
template <typename V, typename Space> struct wrapped_operator : cusp::linear_operator<V, Space> {
    cusp::csr_matrix<int, V, Space> A;
    explicit wrapped_operator(const hcsr<V> &H) : cusp::linear_operator<V, Space>(H.num_rows, H.num_cols, H.num_entries), A(H) {}
    template <typename X, typename Y> void operator()(const X &x, Y &y) const { cusp::multiply(A, x, y); }
};
template <typename V, typename Space> void linear_operator_case()
{
    const hcsr<V> H = poisson_plus_diagonal<V>(10, 10);
    const wrapped_operator<V, Space> A(H);
    const size_t N = H.num_rows;
    cusp::array1d<V, Space> S(1), X = start_vector<V>(N);
    const hvec<V> ones(N, V(1));
    cusp::monitor<V> monitor(ones, kLimit, V(bars<V>::tolerance));
    cusp::precond::diagonal<V, Space> M(A.A);
    cusp::eigen::lobpcg(A, S, X, monitor, M, false);
    outcome o = {monitor.iteration_count(), monitor.converged(), (double)hvec<V>(S)[0], 0, 0};
    measure(H, hvec<V>(X), o.lambda, o);
    // no closed form for A_1: the Rayleigh quotient of a converged x is within residual^2 / gap of an eigenvalue; the Python cases hold the exact value
    expect(o.converged && o.residual <= 2 * bars<V>::tolerance && std::abs(o.x_norm - 1) <= 1e-5 && o.lambda > 1.0 && o.lambda < 4.0, "linear_operator on A_1", o, 0);
}
template <typename Space> void TestLinearOperator()
{
    linear_operator_case<float, Space>();
    linear_operator_case<double, Space>();
}

// X as a column-major array2d with one column; the three-argument overload (default monitor: 500 iterations, 1e-5); S longer than one
template <typename Space> void TestArray2dAndOverloads()
{
    typedef double V;
    const hcsr<V> H = poisson<V>(7, 5);
    const cusp::csr_matrix<int, V, Space> A(H);
    const size_t N = A.num_rows;
    const double want = poisson_eigenvalue(7, 5, false);
    cusp::array2d<V, Space, cusp::column_major> X2(N, 1);
    X2.values = start_vector<V>(N);
    cusp::array1d<V, Space> S(3, V(-1));
    const hvec<V> ones(N, V(1));
    cusp::monitor<V> monitor(ones, kLimit, V(1e-8));
    cusp::eigen::lobpcg(A, S, X2, monitor, false);
    outcome o = {monitor.iteration_count(), monitor.converged(), (double)hvec<V>(S)[0], 0, 0};
    measure(H, hvec<V>(X2.values), o.lambda, o);
    check_outcome(o, want, 1e-8, N, "array2d X");
    ASSERT_TRUE(hvec<V>(S)[1] == V(-1) && hvec<V>(S)[2] == V(-1));
    ASSERT_EQUAL(monitor.residuals.size(), monitor.iteration_count() + 1);
    cusp::array1d<V, Space> X1 = start_vector<V>(N), Xl = start_vector<V>(N);
    cusp::eigen::lobpcg(A, S, X1, false);
    ASSERT_TRUE(std::abs((double)hvec<V>(S)[0] - want) <= 1e-5);
    cusp::eigen::lobpcg(A, S, Xl); // largest is the default
    ASSERT_TRUE(std::abs((double)hvec<V>(S)[0] - poisson_eigenvalue(7, 5, true)) <= 1e-5);
    cusp::array2d<V, Space, cusp::column_major> two(N, 2);
    ASSERT_THROWS(cusp::eigen::lobpcg(A, S, two, monitor, false), cusp::invalid_input_exception);
}

// the loop runs while iteration_count() < min(N, limit): Poisson 7 x 5, largest, double, 1e-9 stops after exactly N = 35 iterations, not converged,
// with S[0] within 1e-10 of the eigenvalue; and a limit below N stops there
template <typename Space> void TestIterationCap()
{
    typedef cusp::csr_matrix<int, double, Space> Csr;
    const hcsr<double> H = poisson<double>(7, 5);
    const outcome o = solve<Csr>(H, 1e-9, true, false);
    expect(o.iterations == 35 && !o.converged && std::abs(o.lambda - poisson_eigenvalue(7, 5, true)) <= 1e-10, "the min(N, limit) cap", o, poisson_eigenvalue(7, 5, true));
    const outcome q = solve<Csr>(H, 1e-9, true, false, 10);
    expect(q.iterations == 10 && !q.converged, "the iteration limit", q, poisson_eigenvalue(7, 5, true));
}

// the breakdown rule: a 3 x 3 gramB that is not positive definite -> the 2 x 2 pair (cp = 0); a 2 x 2 one that is not -> ok == false
template <typename V> void breakdown_rule()
{
    namespace d = cusp::eigen::detail::lobpcg_detail;
    //             <x,aw>  <w,aw>  <x,w>   <x,ap>  <w,ap>  <p,ap>  <x,p>   <w,p>
    const V fine[8] = {V(-0.5), V(3), V(0.125), V(0.25), V(-0.75), V(2.5), V(0.0625), V(-0.25)};
    for (int largest = 0; largest < 2; largest++) {
        const d::ritz<V> full = d::ritz_step(V(1.5), fine, true, largest != 0);
        ASSERT_TRUE(full.ok && full.used_p && full.cp != V(0));
        const d::ritz<V> pair = d::ritz_step(V(1.5), fine, false, largest != 0);
        ASSERT_TRUE(pair.ok && !pair.used_p && pair.cp == V(0));
        V bad_p[8];
        std::copy(fine, fine + 8, bad_p);
        bad_p[6] = V(1.5); // <x,p> = 1.5 between unit vectors: the 3 x 3 gramB is indefinite, its leading 2 x 2 block is fine
        const d::ritz<V> retry = d::ritz_step(V(1.5), bad_p, true, largest != 0);
        ASSERT_TRUE(retry.ok && !retry.used_p && retry.cp == V(0));
        ASSERT_TRUE(retry.lambda == pair.lambda && retry.cx == pair.cx && retry.cr == pair.cr); // exactly the 2 x 2 step
        V bad_w[8];
        std::copy(fine, fine + 8, bad_w);
        bad_w[2] = V(-1.25); // <x,w>: the 2 x 2 block itself is indefinite
        ASSERT_TRUE(!d::ritz_step(V(1.5), bad_w, true, largest != 0).ok && !d::ritz_step(V(1.5), bad_w, false, largest != 0).ok);
        V nan_w[8];
        std::copy(fine, fine + 8, nan_w);
        nan_w[2] = V(NAN);
        ASSERT_TRUE(!d::ritz_step(V(1.5), nan_w, true, largest != 0).ok);
    }
    // the solver leaves lambda, X and the monitor as they stand: X = 0 makes every norm NaN and gramB not positive definite at once
    const hcsr<V> H = poisson<V>(7, 5);
    const cusp::csr_matrix<int, V, TEST_SPACE> A(H);
    cusp::array1d<V, TEST_SPACE> S(1, V(7)), X(35, V(0));
    const hvec<V> ones(35, V(1));
    cusp::monitor<V> monitor(ones, kLimit, V(bars<V>::tolerance));
    cusp::eigen::lobpcg(A, S, X, monitor, false);
    ASSERT_EQUAL(monitor.iteration_count(), (size_t)0);
    ASSERT_TRUE(!monitor.converged());
}
template <typename Space> void TestBreakdownRule()
{
    breakdown_rule<float>();
    breakdown_rule<double>();
}

template <typename Space> void TestShapes()
{
    typedef cusp::csr_matrix<int, float, Space> Csr;
    const Csr A(poisson<float>(4, 4)), R(hcsr<float>(5, 6, 0));
    cusp::array1d<float, Space> S(1), S0(0), X(16, 1.0f), X_short(15, 1.0f), X5(5, 1.0f);
    const hvec<float> ones(16, 1.0f);
    cusp::monitor<float> monitor(ones, 10, 1e-3f);
    ASSERT_THROWS(cusp::eigen::lobpcg(R, S, X5, monitor, false), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::eigen::lobpcg(A, S, X_short, monitor, false), cusp::invalid_input_exception);
    ASSERT_THROWS(cusp::eigen::lobpcg(A, S0, X, monitor, false), cusp::invalid_input_exception);
    ASSERT_EQUAL(monitor.iteration_count(), (size_t)0);
}

// ---- "cases" ---------------------------------------------------------------------------------------------------------------------------------
template <typename V> void print_case(const char *which, const char *kind, size_t m, size_t n, const char *type, double tolerance, const char *precond)
{
    typedef cusp::csr_matrix<int, V, TEST_SPACE> Csr;
    const hcsr<V> H = std::strcmp(kind, "poisson") == 0 ? poisson<V>(m, n) : poisson_plus_diagonal<V>(m, n);
    const bool device = std::strcmp(TEST_SPACE_NAME, "device_memory") == 0;
    const char *runs[3] = {"fused", "fused", "unfused"};
    for (int r = 0; r < (device ? 3 : 1); r++) {
        if (device) setenv("CMI_LOBPCG_FUSED", r == 2 ? "0" : "1", 1);
        const outcome o = solve<Csr>(H, tolerance, std::strcmp(which, "largest") == 0, std::strcmp(precond, "diagonal") == 0);
        std::printf("case %s %s %zux%zu %s %g %s run %s iterations %zu converged %d lambda %a xnorm %a residual %a\n", which, kind, m, n, type, tolerance, precond,
                    device ? runs[r] : "host", o.iterations, (int)o.converged, o.lambda, o.x_norm, o.residual);
    }
    if (device) unsetenv("CMI_LOBPCG_FUSED");
}
inline int print_cases()
{
    print_case<double>("smallest", "poisson", 10, 10, "f64", 1e-8, "identity");
    print_case<double>("smallest", "poisson", 7, 5, "f64", 1e-8, "identity");
    print_case<double>("smallest", "poisson", 33, 31, "f64", 1e-8, "identity");
    print_case<float>("smallest", "poisson", 10, 10, "f32", 1e-3, "identity");
    print_case<float>("smallest", "poisson", 7, 5, "f32", 1e-3, "identity");
    print_case<float>("smallest", "poisson", 33, 31, "f32", 1e-3, "identity");
    print_case<double>("smallest", "a1", 10, 10, "f64", 1e-8, "diagonal");
    print_case<double>("smallest", "a1", 10, 10, "f64", 1e-8, "identity");
    print_case<float>("smallest", "a1", 10, 10, "f32", 1e-3, "diagonal");
    print_case<double>("largest", "poisson", 10, 10, "f64", 1e-8, "identity");
    print_case<double>("largest", "poisson", 33, 31, "f64", 1e-8, "identity");
    return 0;
}

} // namespace lobpcg_check
