// Shared by the multi-shift solver test programs (TEST_SPACE / TEST_SPACE_NAME are defined by the including program): cusp::krylov::cg_m and
// bicgstab_m through the real headers in TEST_SPACE.  The case of the reference's testing/multi_mass.cu -- Poisson 10 x 10 in float, sigma =
// {0.1, 0.5, 1, 5}, monitor (b, 100, 1e-6), every shift's true residual below 1e-4 ||b|| -- for both solvers on all five formats, also on 7 x 5
// (N = 35: every shift after the first is unaligned); the same in double at 1e-10 against 1e-8 ||b|| (the same ratio), also on 33 x 31.  A
// non-symmetric matrix for bicgstab_m, N_s = 1 with sigma = 0, N_s = 0, b = 0, the three invalid_input_exceptions, and the policy dispatch.
#pragma once
#include <cmath>
#include <cstdio>
#include <vector>

#include <cusp/coo_matrix.h>
#include <cusp/csr_matrix.h>
#include <cusp/dia_matrix.h>
#include <cusp/ell_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/hyb_matrix.h>
#include <cusp/krylov/bicgstab_m.h>
#include <cusp/krylov/cg_m.h>

#include "unittest.h"

namespace multishift_check {

template <typename V> using hcsr = cusp::csr_matrix<int, V, cusp::host_memory>;
template <typename V> using hvec = cusp::array1d<V, cusp::host_memory>;
template <typename V> struct bars; // the monitor's tolerance and the residual criterion: 100 x apart, as in testing/multi_mass.cu
template <> struct bars<float> { static constexpr double tolerance = 1e-6, criterion = 1e-4; };
template <> struct bars<double> { static constexpr double tolerance = 1e-10, criterion = 1e-8; };

struct cg_m_solver {
    static const char *name() { return "cg_m"; }
    template <typename A, typename X, typename B, typename S, typename M> static void run(const A &a, X &x, const B &b, const S &s, M &m) { cusp::krylov::cg_m(a, x, b, s, m); }
};
struct bicgstab_m_solver {
    static const char *name() { return "bicgstab_m"; }
    template <typename A, typename X, typename B, typename S, typename M> static void run(const A &a, X &x, const B &b, const S &s, M &m) { cusp::krylov::bicgstab_m(a, x, b, s, m); }
};

// ||b - (A + sigma I) x_s|| / ||b|| in double on the host, whatever space the solve ran in
template <typename V> double relative_residual(const hcsr<V> &A, const hvec<V> &xs, size_t shift, const hvec<V> &b, V sigma)
{
    const size_t N = A.num_rows;
    double rr = 0, bb = 0;
    for (size_t i = 0; i < N; i++) {
        double acc = (double)sigma * (double)xs[shift * N + i];
        for (int jj = A.row_offsets[i]; jj < A.row_offsets[i + 1]; jj++) acc += (double)A.values[jj] * (double)xs[shift * N + A.column_indices[jj]];
        rr += ((double)b[i] - acc) * ((double)b[i] - acc);
        bb += (double)b[i] * (double)b[i];
    }
    return std::sqrt(rr / bb);
}

template <typename Solver, typename Matrix> void solve_and_check(const hcsr<typename Matrix::value_type> &H, const std::vector<double> &shifts, const char *what)
{
    typedef typename Matrix::value_type V;
    const Matrix A(H);
    const size_t N = A.num_rows;
    hvec<V> hs(shifts.size());
    for (size_t s = 0; s < shifts.size(); s++) hs[s] = V(shifts[s]);
    const cusp::array1d<V, TEST_SPACE> sigma(hs), b(N, V(1));
    cusp::array1d<V, TEST_SPACE> x(N * shifts.size(), V(7)); // not zero: the solvers zero-fill x themselves
    cusp::monitor<V> monitor(b, 100, V(bars<V>::tolerance));
    Solver::run(A, x, b, sigma, monitor);
    char msg[256];
    if (!monitor.converged()) {
        std::snprintf(msg, sizeof msg, "%s on %s in %s: not converged after %zu iterations", Solver::name(), what, TEST_SPACE_NAME, monitor.iteration_count());
        throw unittest::failure(msg);
    }
    const hvec<V> hx(x), hb(b);
    for (size_t s = 0; s < shifts.size(); s++) {
        const double rel = relative_residual(H, hx, s, hb, hs[s]);
        if (!(rel < bars<V>::criterion)) {
            std::snprintf(msg, sizeof msg, "%s on %s in %s: sigma = %g has relative residual %.3g, bar %.3g", Solver::name(), what, TEST_SPACE_NAME, shifts[s], rel,
                          bars<V>::criterion);
            throw unittest::failure(msg);
        }
    }
}

template <typename V> hcsr<V> poisson(size_t m, size_t n)
{
    hcsr<V> A;
    cusp::gallery::poisson5pt(A, m, n);
    return A;
}
// 100 x 100, non-symmetric, strictly diagonally dominant: 4 on the diagonal, -1.5 / -0.5 beside it, -0.7 / -0.3 ten columns away
template <typename V> hcsr<V> nonsymmetric100()
{
    const int N = 100;
    cusp::coo_matrix<int, V, cusp::host_memory> C(N, N, 0);
    std::vector<int> I, J;
    std::vector<V> X;
    for (int i = 0; i < N; i++) {
        const int cols[5] = {i - 10, i - 1, i, i + 1, i + 10};
        const double vals[5] = {-0.3, -0.5, 4.0, -1.5, -0.7};
        for (int k = 0; k < 5; k++)
            if (cols[k] >= 0 && cols[k] < N) { I.push_back(i); J.push_back(cols[k]); X.push_back(V(vals[k])); }
    }
    C.resize(N, N, I.size());
    for (size_t k = 0; k < I.size(); k++) { C.row_indices[k] = I[k]; C.column_indices[k] = J[k]; C.values[k] = X[k]; }
    return hcsr<V>(C);
}

const std::vector<double> kShifts = {0.1, 0.5, 1.0, 5.0};

// the multi_mass.cu case and its neighbours: every format x value type, both solvers
template <typename Matrix> void TestMultiMass()
{
    typedef typename Matrix::value_type V;
    solve_and_check<cg_m_solver, Matrix>(poisson<V>(10, 10), kShifts, "poisson10x10");
    solve_and_check<bicgstab_m_solver, Matrix>(poisson<V>(10, 10), kShifts, "poisson10x10");
    solve_and_check<cg_m_solver, Matrix>(poisson<V>(7, 5), kShifts, "poisson7x5");
    solve_and_check<bicgstab_m_solver, Matrix>(poisson<V>(7, 5), kShifts, "poisson7x5");
    if (std::is_same<V, double>::value) { // (float: a long-converged shift turns NaN in bicgstab_m there -- the reference's arithmetic)
        solve_and_check<cg_m_solver, Matrix>(poisson<V>(33, 31), kShifts, "poisson33x31");
        solve_and_check<bicgstab_m_solver, Matrix>(poisson<V>(33, 31), kShifts, "poisson33x31");
    }
}

template <typename V, typename Space> void nonsymmetric()
{
    solve_and_check<bicgstab_m_solver, cusp::csr_matrix<int, V, Space>>(nonsymmetric100<V>(), {0.0, 0.3, 2.0}, "nonsymmetric100");
    solve_and_check<bicgstab_m_solver, cusp::coo_matrix<int, V, Space>>(nonsymmetric100<V>(), {0.0, 0.3, 2.0}, "nonsymmetric100");
}
template <typename Space> void TestNonSymmetric()
{
    nonsymmetric<float, Space>();
    nonsymmetric<double, Space>();
}

template <typename V, typename Space> void edge_cases()
{
    typedef cusp::csr_matrix<int, V, Space> Csr;
    typedef cusp::array1d<V, Space> Vec;
    const hcsr<V> H = poisson<V>(10, 10);
    const Csr A(H);
    const size_t N = A.num_rows;
    // one shift, sigma = 0: A x = b
    solve_and_check<cg_m_solver, Csr>(H, {0.0}, "poisson10x10, sigma = {0}");
    solve_and_check<bicgstab_m_solver, Csr>(H, {0.0}, "poisson10x10, sigma = {0}");
    // no shift at all: the base recurrence runs against the monitor, x stays empty
    {
        const Vec b(N, V(1)), sigma(0);
        Vec x(0);
        cusp::monitor<V> m1(b, 100, V(bars<V>::tolerance)), m2(b, 100, V(bars<V>::tolerance));
        cusp::krylov::cg_m(A, x, b, sigma, m1);
        cusp::krylov::bicgstab_m(A, x, b, sigma, m2);
        ASSERT_TRUE(m1.converged() && m1.iteration_count() > 0 && m2.converged() && m2.iteration_count() > 0);
        ASSERT_EQUAL(x.size(), (size_t)0);
    }
    // b = 0: satisfied at entry -- x is zero-filled, no iteration, no NaN
    {
        hvec<V> hs(2);
        hs[0] = V(0.5);
        hs[1] = V(2);
        const Vec b(N, V(0)), sigma(hs);
        Vec x1(2 * N, V(3)), x2(2 * N, V(3));
        cusp::monitor<V> m1(b, 100, V(bars<V>::tolerance)), m2(b, 100, V(bars<V>::tolerance));
        cusp::krylov::cg_m(A, x1, b, sigma, m1);
        cusp::krylov::bicgstab_m(A, x2, b, sigma, m2);
        ASSERT_EQUAL(m1.iteration_count(), (size_t)0);
        ASSERT_EQUAL(m2.iteration_count(), (size_t)0);
        const hvec<V> h1(x1), h2(x2);
        for (size_t i = 0; i < 2 * N; i++) ASSERT_TRUE(h1[i] == V(0) && h2[i] == V(0));
    }
    // what the reference asserts is thrown here
    {
        const Vec b(N, V(1)), sigma(2, V(1)), b_short(N - 1, V(1));
        Vec x(2 * N), x_short(2 * N - 1);
        cusp::monitor<V> m(b, 10, V(1e-3));
        const Csr R(hcsr<V>(5, 6, 0));
        const Vec b5(5, V(1));
        Vec x10(10);
        ASSERT_THROWS(cusp::krylov::cg_m(R, x10, b5, sigma, m), cusp::invalid_input_exception);
        ASSERT_THROWS(cusp::krylov::cg_m(A, x, b_short, sigma, m), cusp::invalid_input_exception);
        ASSERT_THROWS(cusp::krylov::cg_m(A, x_short, b, sigma, m), cusp::invalid_input_exception);
        ASSERT_THROWS(cusp::krylov::bicgstab_m(R, x10, b5, sigma, m), cusp::invalid_input_exception);
        ASSERT_THROWS(cusp::krylov::bicgstab_m(A, x, b_short, sigma, m), cusp::invalid_input_exception);
        ASSERT_THROWS(cusp::krylov::bicgstab_m(A, x_short, b, sigma, m), cusp::invalid_input_exception);
    }
}
template <typename Space> void TestEdgeCases()
{
    edge_cases<float, Space>();
    edge_cases<double, Space>();
}

// a user policy: its overloads are reached by ADL and nothing is solved; a policy without overloads gets the default
struct my_policy : cusp::execution_policy<my_policy> { int hits = 0; };
template <typename A, typename X, typename B, typename S, typename M> void cg_m(my_policy &p, const A &, X &, const B &, const S &, M &) { p.hits += 1; }
template <typename A, typename X, typename B, typename S, typename M> void bicgstab_m(my_policy &p, const A &, X &, const B &, const S &, M &) { p.hits += 10; }
template <typename A, typename X, typename B, typename S> void bicgstab_m(my_policy &p, const A &, X &, const B &, const S &) { p.hits += 100; }
struct plain_policy : cusp::execution_policy<plain_policy> {};

template <typename Space> void TestPolicyDispatch()
{
    typedef cusp::csr_matrix<int, float, Space> Csr;
    const hcsr<float> H = poisson<float>(10, 10);
    const Csr A(H);
    const size_t N = A.num_rows;
    const cusp::array1d<float, Space> b(N, 1.0f), sigma(1, 0.5f);
    cusp::array1d<float, Space> x(N, 9.0f);
    cusp::monitor<float> monitor(b, 100, 1e-6f);
    my_policy mine;
    cusp::krylov::cg_m(mine, A, x, b, sigma, monitor);
    ASSERT_EQUAL(mine.hits, 1);
    cusp::krylov::bicgstab_m(mine, A, x, b, sigma, monitor);
    ASSERT_EQUAL(mine.hits, 11);
    cusp::krylov::bicgstab_m(mine, A, x, b, sigma);
    ASSERT_EQUAL(mine.hits, 111);
    ASSERT_EQUAL(monitor.iteration_count(), (size_t)0);
    plain_policy plain;
    cusp::krylov::cg_m(plain, A, x, b, sigma, monitor);
    ASSERT_TRUE(monitor.converged() && monitor.iteration_count() > 0);
    ASSERT_TRUE(relative_residual(H, hvec<float>(x), 0, hvec<float>(b), 0.5f) < 1e-4);
    cusp::monitor<float> monitor2(b, 100, 1e-6f);
    cusp::krylov::bicgstab_m(plain, A, x, b, sigma, monitor2);
    ASSERT_TRUE(monitor2.converged() && relative_residual(H, hvec<float>(x), 0, hvec<float>(b), 0.5f) < 1e-4);
    cusp::krylov::cg_m(plain, A, x, b, sigma);      // the default monitors (b, 500, 1e-5)
    cusp::krylov::bicgstab_m(plain, A, x, b, sigma);
    cusp::krylov::cg_m(A, x, b, sigma);
    cusp::krylov::bicgstab_m(A, x, b, sigma);
    ASSERT_TRUE(relative_residual(H, hvec<float>(x), 0, hvec<float>(b), 0.5f) < 1e-3);
}

} // namespace multishift_check
