// Shared by the AINV test programs: the reference's test cases (testing/ainv.cu) as templates over the memory space and the value type, the
// heap test, the problems both memory spaces factor, and the dump the Python side compares with tests/ainv_refs.py bit for bit.
#pragma once
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include <cusp/coo_matrix.h>
#include <cusp/csr_matrix.h>
#include <cusp/detail/random_hash.h>
#include <cusp/dia_matrix.h>
#include <cusp/ell_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/hyb_matrix.h>
#include <cusp/krylov/cg.h>
#include <cusp/monitor.h>
#include <cusp/precond/ainv.h>

#include "unittest.h"

namespace ainv_check {

template <typename V> using host_csr = cusp::csr_matrix<int, V, cusp::host_memory>;

template <typename V> uint64_t bits_of(V v)
{
    typename std::conditional<sizeof(V) == 8, uint64_t, uint32_t>::type u;
    std::memcpy(&u, &v, sizeof(V));
    return u;
}

// poisson5pt(m, n) with values[0] = 10, the reference tests' matrix
template <typename Matrix> Matrix problem(size_t m, size_t n)
{
    host_csr<typename Matrix::value_type> A;
    cusp::gallery::poisson5pt(A, m, n);
    A.values[0] = 10;
    return Matrix(A);
}
// ... and a matrix that is not symmetric: the same with every entry above the diagonal halved
template <typename V> host_csr<V> nonsymmetric_problem(size_t m, size_t n)
{
    host_csr<V> A = problem<host_csr<V>>(m, n);
    for (size_t i = 0; i < A.num_rows; i++)
        for (int e = A.row_offsets[i]; e < A.row_offsets[i + 1]; e++)
            if ((size_t)A.column_indices[e] > i) A.values[e] = A.values[e] * V(0.5);
    return A;
}

// x[i] uniform in [0, 1) from the library's hash
template <typename V, typename Space> cusp::array1d<V, Space> start_vector(size_t n)
{
    cusp::array1d<V, cusp::host_memory> x(n);
    for (size_t i = 0; i < n; i++) x[i] = cusp::detail::random_unit(cusp::detail::random_hash(i, 100), (V *)nullptr);
    return cusp::array1d<V, Space>(x);
}

// the reference's heap test with fewer trials: insert 100, update all, remove half, insert 100 more, then both validators
inline void heap_test(int trials)
{
    uint64_t seed = 100;
    auto rng = [&] { return cusp::detail::random_unit(cusp::detail::random_hash(seed++, 7), (float *)nullptr); };
    for (int trial = 0; trial < trials; trial++) {
        cusp::precond::detail::ainv_matrix_row<int, float> row;
        const int size = 100;
        for (int i = 0; i < size; i++) row.insert(i, rng());
        for (int i = 0; i < size; i++) row.add_to_value(i, rng() - .5f);
        ASSERT_EQUAL(row.validate_heap(), true);
        for (int i = 0; i < size / 2; i++) row.remove_min();
        ASSERT_EQUAL(row.size(), (size_t)(size / 2));
        for (int i = 0; i < size; i++) row.insert(i + size, rng());
        ASSERT_EQUAL(row.validate_heap(), true);
        ASSERT_EQUAL(row.validate_backpointers(), true);
        ASSERT_EQUAL(row.has_entry_at_index(size), true);
    }
}

struct solve_result {
    bool converged;
    size_t iterations;
    double residual;
};
// cg on A x = 0 from the hashed start with M, to an absolute residual of 1e-5 within `limit` iterations
template <typename V, typename Space, typename Matrix, typename Precond> solve_result solve(const Matrix &A, Precond &M, size_t limit)
{
    cusp::array1d<V, Space> x = start_vector<V, Space>(A.num_rows), b(A.num_rows, V(0));
    cusp::monitor<V> monitor(b, limit, 0, 1e-5);
    cusp::krylov::cg(A, x, b, monitor, M);
    return {monitor.converged(), monitor.iteration_count(), (double)monitor.residual_norm()};
}

// TestAINVFactorization: after the exact factorisation cg converges within 1 iteration
template <typename V, typename Space> void exact_factorisation_case()
{
    typedef cusp::csr_matrix<int, V, Space> Matrix;
    const Matrix A = problem<Matrix>(10, 10);
    cusp::precond::scaled_bridson_ainv<V, Space> M(A, 0, -1);
    ASSERT_EQUAL((solve<V, Space>(A, M, 1).converged), true);
}
// TestAINVSymmetry: on a symmetric matrix the symmetric and the non-symmetric class end with EQUAL residual norms
template <typename V, typename Space> void symmetry_case()
{
    typedef cusp::csr_matrix<int, V, Space> Matrix;
    const Matrix A = problem<Matrix>(100, 100);
    cusp::precond::bridson_ainv<V, Space> M1(A, .1);
    cusp::precond::nonsym_bridson_ainv<V, Space> M2(A, .1);
    const solve_result r1 = solve<V, Space>(A, M1, 125), r2 = solve<V, Space>(A, M2, 125);
    ASSERT_EQUAL(r1.converged, true);
    ASSERT_EQUAL(r2.converged, true);
    ASSERT_EQUAL(r1.residual, r2.residual);
    ASSERT_EQUAL(r1.iterations, r2.iterations);
}
// TestAINVConvergence: the eight cases within the reference's iteration limits
template <typename V, typename Space, template <typename, typename> class Precond> void convergence_cases(const char *name)
{
    typedef cusp::csr_matrix<int, V, Space> Matrix;
    const Matrix A = problem<Matrix>(100, 100);
    struct { V tol; int per_row; bool lin; int lin_param; size_t limit; } cases[4] = {{V(.1), -1, false, 1, 125}, {0, 10, false, 1, 70}, {V(.01), 4, false, 1, 120}, {0, -1, true, 4, 120}};
    for (const auto &c : cases) {
        Precond<V, Space> M(A, c.tol, c.per_row, c.lin, c.lin_param);
        const solve_result r = solve<V, Space>(A, M, c.limit);
        std::printf("%s<%s>(%g, %d, %d, %d): %zu iterations (limit %zu), residual %.3e\n", name, sizeof(V) == 8 ? "double" : "float", (double)c.tol, c.per_row, (int)c.lin, c.lin_param,
                    r.iterations, c.limit, r.residual);
        ASSERT_EQUAL(r.converged, true);
    }
}

// the dropping settings of the dump: the reference tests' four and one whose Lin-More bound falls to its floor of 1
struct setting { double tol; int per_row; bool lin; int lin_param; };
inline const std::vector<setting> &settings()
{
    static const std::vector<setting> s = {{.1, -1, false, 1}, {0, 10, false, 1}, {.01, 4, false, 1}, {0, -1, true, 4}, {0, -1, true, -10}};
    return s;
}

template <typename V, typename Hyb> void print_matrix(const char *what, const Hyb &m)
{
    const host_csr<V> c(m);
    std::printf("M %s %zu %zu\n", what, c.num_rows, c.num_entries);
    for (size_t i = 0; i <= c.num_rows; i++) std::printf("%d ", (int)c.row_offsets[i]);
    std::printf("\n");
    for (size_t e = 0; e < c.num_entries; e++) std::printf("%d %" PRIx64 "\n", (int)c.column_indices[e], bits_of<V>(c.values[e]));
}
template <typename V, typename Array> void print_vector(const char *what, const Array &a)
{
    const cusp::array1d<V, cusp::host_memory> h(a);
    std::printf("D %s %zu\n", what, h.size());
    for (size_t i = 0; i < h.size(); i++) std::printf("%" PRIx64 " ", bits_of<V>(h[i]));
    std::printf("\n");
}
// "--dump f64|f32": every class on poisson5pt 33 x 31 (values[0] = 10) and nonsym_bridson_ainv on the non-symmetric 7 x 5, every setting
template <typename V> int dump()
{
    const host_csr<V> A = problem<host_csr<V>>(33, 31), B = nonsymmetric_problem<V>(7, 5);
    for (size_t k = 0; k < settings().size(); k++) {
        const setting &s = settings()[k];
        std::printf("S %zu\n", k);
        {
            cusp::precond::scaled_bridson_ainv<V, cusp::host_memory> M(A, (V)s.tol, s.per_row, s.lin, s.lin_param);
            print_matrix<V>("scaled.w", M.w);
            print_matrix<V>("scaled.w_t", M.w_t);
        }
        {
            cusp::precond::bridson_ainv<V, cusp::host_memory> M(A, (V)s.tol, s.per_row, s.lin, s.lin_param);
            print_matrix<V>("bridson.w", M.w);
            print_matrix<V>("bridson.w_t", M.w_t);
            print_vector<V>("bridson.diagonals", M.diagonals);
        }
        for (int which = 0; which < 2; which++) {
            cusp::precond::nonsym_bridson_ainv<V, cusp::host_memory> M(which ? B : A, (V)s.tol, s.per_row, s.lin, s.lin_param);
            print_matrix<V>(which ? "nonsym7x5.z" : "nonsym.z", M.z);
            print_matrix<V>(which ? "nonsym7x5.w_t" : "nonsym.w_t", M.w_t);
            print_vector<V>(which ? "nonsym7x5.diagonals" : "nonsym.diagonals", M.diagonals);
        }
    }
    return 0;
}

} // namespace ainv_check
