// Shared by the Gauss-Seidel test programs: the cases of the reference's testing/gauss_seidel.cu as templates over the memory
// space (float, as there, and double), cusp::graph::vertex_coloring on the reference's matrix and on the 5-point stencil, a
// naive restatement of the sweep on a host CSR matrix (plain loops over colour lists built here; one rounding per operation),
// and checks of cusp::relaxation::gauss_seidel / sor in TEST_SPACE against it bit for bit -- on symmetric and non-symmetric
// patterns, with rows without a diagonal, stored zeros and a diagonal stored twice.
// TEST_SPACE / TEST_SPACE_NAME are defined by the including program.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include <cusp/array2d.h>
#include <cusp/coo_matrix.h>
#include <cusp/csr_matrix.h>
#include <cusp/gallery/poisson.h>
#include <cusp/graph/vertex_coloring.h>
#include <cusp/relaxation/gauss_seidel.h>
#include <cusp/relaxation/sor.h>

#include "unittest.h"

namespace gs_check {

using cusp::relaxation::BACKWARD;
using cusp::relaxation::FORWARD;
using cusp::relaxation::SYMMETRIC;
template <typename V> using hvec = cusp::array1d<V, cusp::host_memory>;
template <typename V> using hcsr = cusp::csr_matrix<int, V, cusp::host_memory>;

// seeded values in [-8, 8) with a fractional part: products and sums round, so order and contraction show in the bits
inline double seeded(uint64_t i)
{
    uint64_t z = i * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull;
    z ^= z >> 31; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 29;
    return (double)(z % 4096) / 256.0 - 8.0 + 1.0 / 3.0;
}
template <typename V> hvec<V> seeded_vector(size_t n, uint64_t salt)
{
    hvec<V> v(n);
    for (size_t i = 0; i < n; i++) v[i] = (V)seeded(salt + 131 * i);
    return v;
}
// same bits; a NaN equals a NaN whatever its sign and payload
template <typename A, typename B> bool bits_equal(const A &a, const B &b)
{
    typedef typename A::value_type V;
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); i++) {
        const V x = a[i], y = b[i];
        if (x != x && y != y) continue;
        if (std::memcmp(&x, &y, sizeof(V)) != 0) return false;
    }
    return true;
}
template <typename V> cusp::array2d<V, cusp::host_memory> dense(size_t n, std::vector<double> v)
{
    cusp::array2d<V, cusp::host_memory> a(n, n);
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < n; j++) a(i, j) = (V)v[i * n + j];
    return a;
}
inline std::vector<double> reference_5x5() { return {1, 1, 2, 0, 0, 3, 2, 0, 0, 5, 0, 0, 0.5, 0, 0, 0, 6, 7, 4, 0, 0, 8, 0, 0, 8}; }

// a host CSR matrix from per-row (column, value) lists
template <typename V> hcsr<V> from_rows(const std::vector<std::vector<std::pair<int, double>>> &rows)
{
    size_t nnz = 0;
    for (const auto &r : rows) nnz += r.size();
    hcsr<V> A(rows.size(), rows.size(), nnz);
    size_t p = 0;
    for (size_t i = 0; i < rows.size(); i++) {
        A.row_offsets[i] = (int)p;
        for (const auto &e : rows[i]) { A.column_indices[p] = e.first; A.values[p] = (V)e.second; p++; }
    }
    A.row_offsets[rows.size()] = (int)p;
    return A;
}
// n rows, each with up to `per_row` seeded off-diagonal columns anywhere (so the pattern is NOT symmetric) and, by row index:
// i % 11 == 3 no diagonal, == 5 a stored zero, == 7 a stored -0, == 9 the diagonal stored twice (first, and again last), else once
template <typename V> hcsr<V> irregular(size_t n, size_t per_row, uint64_t salt)
{
    std::vector<std::vector<std::pair<int, double>>> rows(n);
    for (size_t i = 0; i < n; i++) {
        std::vector<int> cols;
        for (size_t k = 0; k < per_row; k++) {
            const int j = (int)((uint64_t)(seeded(salt + 977 * i + k) * 256.0 + 4096.0) * 2654435761ull % n);
            if ((size_t)j != i && std::find(cols.begin(), cols.end(), j) == cols.end()) cols.push_back(j);
        }
        std::sort(cols.begin(), cols.end());
        const double d = 4.0 + std::abs(seeded(salt + 31 * i));
        auto &r = rows[i];
        if (i % 11 == 9) r.push_back({(int)i, 100.0});
        for (int j : cols) r.push_back({j, seeded(salt + 7 * i + j)});
        if (i % 11 == 5) r.push_back({(int)i, 0.0});
        else if (i % 11 == 7) r.push_back({(int)i, -0.0});
        else if (i % 11 != 3) r.push_back({(int)i, d});
    }
    return from_rows<V>(rows);
}

// ---- naive restatements on a host CSR matrix ----
struct naive_schedule {
    std::vector<int> colors;
    std::vector<std::vector<int>> rows_of; // per colour, ascending
    bool conflict = false;                 // some row holds an off-diagonal column of its own colour
};
template <typename V> naive_schedule naive_colouring(const hcsr<V> &A)
{
    const size_t n = A.num_rows;
    naive_schedule s;
    s.colors.assign(n, (int)n - 1);
    std::vector<long long> mark(n ? n : 1, -1);
    size_t count = 0;
    for (size_t v = 0; v < n; v++) {
        for (int jj = A.row_offsets[v]; jj < A.row_offsets[v + 1]; jj++) mark[s.colors[A.column_indices[jj]]] = (long long)v;
        size_t c = 0;
        while (c < count && mark[c] == (long long)v) c++;
        if (c == count) count++;
        s.colors[v] = (int)c;
    }
    s.rows_of.resize(count);
    for (size_t v = 0; v < n; v++) s.rows_of[s.colors[v]].push_back((int)v);
    for (size_t v = 0; v < n; v++)
        for (int jj = A.row_offsets[v]; jj < A.row_offsets[v + 1]; jj++)
            if ((size_t)A.column_indices[jj] != v && s.colors[A.column_indices[jj]] == s.colors[v]) s.conflict = true;
    return s;
}
template <typename V> void naive_colour(const hcsr<V> &A, const hvec<V> &b, hvec<V> &x, const std::vector<int> &rows)
{
    for (int i : rows) {
        V rsum = V(0), diag = V(0);
        for (int jj = A.row_offsets[i]; jj < A.row_offsets[i + 1]; jj++) {
            const int j = A.column_indices[jj];
            if (j == i) { diag = A.values[jj]; continue; }
            const V p = A.values[jj] * x[j];
            rsum = rsum + p;
        }
        if (diag != V(0)) {
            const V d = b[i] - rsum;
            x[i] = d / diag;
        }
    }
}
template <typename V> hvec<V> naive_sweep(const hcsr<V> &A, const hvec<V> &b, hvec<V> x, cusp::relaxation::sweep direction)
{
    const naive_schedule s = naive_colouring(A);
    const size_t C = s.rows_of.size();
    if (direction != BACKWARD)
        for (size_t c = 0; c < C; c++) naive_colour(A, b, x, s.rows_of[c]);
    if (direction != FORWARD)
        for (size_t c = C; c > 0; c--) naive_colour(A, b, x, s.rows_of[c - 1]);
    return x;
}
template <typename V> hvec<V> naive_sor(const hcsr<V> &A, const hvec<V> &b, const hvec<V> &x, V omega, cusp::relaxation::sweep direction)
{
    const hvec<V> swept = naive_sweep(A, b, x, direction);
    hvec<V> out(x.size());
    const V keep = V(1) - omega;
    for (size_t i = 0; i < x.size(); i++) { const V p = keep * x[i], q = omega * swept[i]; out[i] = p + q; }
    return out;
}

// ---- the reference's cases (testing/gauss_seidel.cu), in float as there and in double ----
template <typename V, typename Space> void reference_relaxation()
{
    cusp::csr_matrix<int, V, Space> A(dense<V>(5, reference_5x5()));
    cusp::array1d<V, Space> b(5, V(5)), x(5, V(-1));
    cusp::relaxation::gauss_seidel<V, Space> relax(A);
    ASSERT_EQUAL(relax.default_direction, SYMMETRIC);
    ASSERT_EQUAL(relax.color_offsets.size(), (size_t)4);
    const int order[5] = {0, 2, 4, 1, 3}, offsets[4] = {0, 3, 4, 5};
    cusp::array1d<int, cusp::host_memory> ho(relax.ordering);
    for (int i = 0; i < 5; i++) ASSERT_EQUAL(ho[i], order[i]);
    for (int i = 0; i < 4; i++) ASSERT_EQUAL(relax.color_offsets[i], offsets[i]);
    ASSERT_EQUAL(relax.color_conflicts[0], 1); // rows 0 and 2 share colour 0 and row 0 holds column 2
    ASSERT_EQUAL(relax.color_conflicts[1], 0);
    ASSERT_EQUAL(relax.color_conflicts[2], 0);
    ASSERT_EQUAL(relax.scratch.size(), (size_t)3);
    relax(A, b, x);
    const V want[5] = {-1.4375, -13.5625, 10, 4.09375, 14.1875}; // every step is exact in binary: equality, not a tolerance
    hvec<V> got(x);
    for (int i = 0; i < 5; i++) ASSERT_EQUAL(got[i], want[i]);
    // SOR on the same data: omega = 1 is the sweep, omega = 0.5 the mean of the sweep and the start (tests/gauss_seidel_refs.py)
    cusp::array1d<V, Space> x1(5, V(-1)), xh(5, V(-1));
    cusp::relaxation::sor<V, Space> one(A, V(1)), half(A, V(0.5));
    one(A, b, x1);
    half(A, b, xh);
    hvec<V> g1(x1), gh(xh);
    for (int i = 0; i < 5; i++) { ASSERT_EQUAL(g1[i], want[i]); ASSERT_EQUAL(gh[i], V(0.5) * V(-1) + V(0.5) * want[i]); }
    std::printf("SOR5 %s %s:", sizeof(V) == 8 ? "f64" : "f32", TEST_SPACE_NAME);
    cusp::array1d<V, Space> xs(5, V(-1));
    cusp::relaxation::sor<V, Space> s15(A, V(1.5), FORWARD);
    s15(A, b, xs);
    hvec<V> gs(xs);
    for (int i = 0; i < 5; i++) std::printf(" %a", (double)gs[i]);
    std::printf("\n");
}
template <typename Space> void TestGaussSeidelRelaxation()
{
    reference_relaxation<float, Space>();
    reference_relaxation<double, Space>();
}
template <typename V, typename Space> void reference_sweeps()
{
    cusp::csr_matrix<int, V, Space> A(dense<V>(2, {2, 1, 1, 3}));
    {
        cusp::array1d<V, Space> b(2, V(5)), x(2, V(-1));
        cusp::relaxation::gauss_seidel<V, Space> relax(A);
        relax(A, b, x, FORWARD);
        hvec<V> got(x);
        ASSERT_EQUAL(got[0], V(3));
        ASSERT_EQUAL(got[1], V(2) / V(3));
    }
    {
        cusp::array1d<V, Space> b(2, V(5)), x(2, V(-1));
        cusp::relaxation::gauss_seidel<V, Space> relax(A, FORWARD);
        ASSERT_EQUAL(relax.default_direction, FORWARD);
        relax(A, b, x, BACKWARD);
        hvec<V> got(x);
        ASSERT_EQUAL(got[0], V(1.5));
        ASSERT_EQUAL(got[1], V(2));
    }
}
template <typename Space> void TestGaussSeidelRelaxationSweeps()
{
    reference_sweeps<float, Space>();
    reference_sweeps<double, Space>();
}

// ---- colouring ----
template <typename Space> void TestVertexColoring()
{
    cusp::csr_matrix<int, float, Space> A(dense<float>(5, reference_5x5()));
    cusp::array1d<int, Space> colors;
    ASSERT_EQUAL(cusp::graph::vertex_coloring(A, colors), (size_t)3);
    const int want[5] = {0, 1, 0, 2, 0};
    cusp::array1d<int, cusp::host_memory> hc(colors);
    ASSERT_EQUAL(hc.size(), (size_t)5);
    for (int i = 0; i < 5; i++) ASSERT_EQUAL(hc[i], want[i]);
    // another format goes through cusp::convert's host CSR: the same colours
    cusp::coo_matrix<int, float, Space> C(A);
    cusp::array1d<int, cusp::host_memory> cc;
    ASSERT_EQUAL(cusp::graph::vertex_coloring(C, cc), (size_t)3);
    for (int i = 0; i < 5; i++) ASSERT_EQUAL(cc[i], want[i]);
    // the 5-point stencil on 10 x 10: two colours, red-black
    cusp::csr_matrix<int, double, Space> P;
    cusp::gallery::poisson5pt(P, 10, 10);
    cusp::array1d<int, Space> pc(100);
    ASSERT_EQUAL(cusp::graph::vertex_coloring(P, pc), (size_t)2);
    cusp::array1d<int, cusp::host_memory> hp(pc);
    for (int i = 0; i < 100; i++) ASSERT_EQUAL(hp[i], (i % 10 + i / 10) % 2);
    cusp::relaxation::gauss_seidel<double, Space> relax(P);
    ASSERT_EQUAL(relax.color_offsets.size(), (size_t)3);
    ASSERT_EQUAL(relax.color_offsets[1], 50);
    ASSERT_EQUAL(relax.color_conflicts[0] + relax.color_conflicts[1], 0);
    ASSERT_EQUAL(relax.scratch.size(), (size_t)0);
    // not square
    cusp::csr_matrix<int, float, Space> R(2, 3, 0);
    ASSERT_THROWS(cusp::graph::vertex_coloring(R, colors), cusp::invalid_input_exception);
    // empty
    cusp::csr_matrix<int, float, Space> E(0, 0, 0);
    ASSERT_EQUAL(cusp::graph::vertex_coloring(E, colors), (size_t)0);
    ASSERT_EQUAL(colors.size(), (size_t)0);
}

// ---- the classes against the naive restatement: bit for bit ----
template <typename V, typename Space> void check_against_naive(const hcsr<V> &H, uint64_t salt, bool expect_conflict)
{
    const size_t n = H.num_rows;
    cusp::csr_matrix<int, V, Space> A(H);
    const hvec<V> hb = seeded_vector<V>(n, salt + 1), hx = seeded_vector<V>(n, salt + 2);
    const cusp::array1d<V, Space> b(hb);
    const naive_schedule s = naive_colouring(H);
    ASSERT_EQUAL(s.conflict, expect_conflict);
    cusp::relaxation::gauss_seidel<V, Space> relax(A);
    ASSERT_EQUAL(relax.color_offsets.size(), s.rows_of.size() + 1);
    int flagged = 0;
    for (size_t c = 0; c < relax.color_conflicts.size(); c++) flagged += relax.color_conflicts[c];
    ASSERT_EQUAL(flagged > 0, expect_conflict);
    const cusp::relaxation::sweep dirs[3] = {FORWARD, BACKWARD, SYMMETRIC};
    for (int d = 0; d < 3; d++) {
        cusp::array1d<V, Space> x(hx);
        const V *where = x.data();
        relax(A, b, x, dirs[d]);
        ASSERT_TRUE(x.data() == where);
        const hvec<V> once = naive_sweep(H, hb, hx, dirs[d]);
        ASSERT_TRUE(bits_equal(hvec<V>(x), once));
        relax(A, b, x, dirs[d]); // a second sweep on the same object: the scratch carries no state
        ASSERT_TRUE(bits_equal(hvec<V>(x), naive_sweep(H, hb, once, dirs[d])));
        cusp::relaxation::sor<V, Space> sor(A, V(1.5), dirs[d]);
        cusp::array1d<V, Space> xs(hx);
        sor(A, b, xs);
        ASSERT_TRUE(bits_equal(hvec<V>(xs), naive_sor(H, hb, hx, V(1.5), dirs[d])));
        sor(A, b, xs, V(0.7), dirs[2 - d]);
        ASSERT_TRUE(bits_equal(hvec<V>(xs), naive_sor(H, hb, naive_sor(H, hb, hx, V(1.5), dirs[d]), V(0.7), dirs[2 - d])));
    }
    // a copy in the other memory space does the same work in its own space's way
    {
        cusp::relaxation::gauss_seidel<V, cusp::host_memory> on_host(relax);
        ASSERT_TRUE(bits_equal(hvec<V>(on_host.diagonal), hvec<V>(relax.diagonal)));
        hvec<V> x(hx);
        on_host(H, hb, x, SYMMETRIC);
        ASSERT_TRUE(bits_equal(x, naive_sweep(H, hb, hx, SYMMETRIC)));
        cusp::relaxation::gauss_seidel<V, Space> back(on_host);
        cusp::array1d<V, Space> xb(hx);
        back(A, b, xb);
        ASSERT_TRUE(bits_equal(hvec<V>(xb), naive_sweep(H, hb, hx, SYMMETRIC)));
    }
}
template <typename V, typename Space> void against_naive()
{
    hcsr<V> P;
    cusp::gallery::poisson5pt(P, 23, 17); // 391 rows, two colours of 196 and 195
    for (size_t k = 0; k < P.num_entries; k++) P.values[k] = (V)seeded(5 + 7 * k);
    check_against_naive<V, Space>(P, 11, false);
    check_against_naive<V, Space>(irregular<V>(200, 6, 3), 13, true);  // a non-symmetric pattern: colours whose rows depend on one another
    check_against_naive<V, Space>(irregular<V>(70, 40, 4), 17, true);  // long rows, many colours
    hcsr<V> one(1, 1, 1);
    one.row_offsets[0] = 0; one.row_offsets[1] = 1; one.column_indices[0] = 0; one.values[0] = V(3);
    check_against_naive<V, Space>(one, 19, false);
}
template <typename Space> void TestAgainstNaive()
{
    against_naive<float, Space>();
    against_naive<double, Space>();
}

template <typename Space> void TestArgumentErrors()
{
    hcsr<double> H;
    cusp::gallery::poisson5pt(H, 4, 3);
    cusp::csr_matrix<int, double, Space> A(H);
    cusp::array1d<double, Space> b(12, 1.0), x(12, 1.0), shorter(11, 1.0);
    cusp::relaxation::gauss_seidel<double, Space> relax(A);
    ASSERT_THROWS(relax(A, shorter, x), cusp::invalid_input_exception);
    ASSERT_THROWS(relax(A, b, shorter), cusp::invalid_input_exception);
    ASSERT_THROWS(relax(A, b, x, (cusp::relaxation::sweep)7), cusp::runtime_exception);
    cusp::csr_matrix<int, double, Space> other(cusp::csr_matrix<int, double, cusp::host_memory>(5, 5, 0));
    cusp::array1d<double, Space> b5(5, 1.0), x5(5, 1.0);
    ASSERT_THROWS(relax(other, b5, x5), cusp::invalid_input_exception); // not the matrix the object was made from
    cusp::relaxation::sor<double, Space> sor(A, 1.2);
    ASSERT_THROWS(sor(A, b, shorter), cusp::invalid_input_exception);
    ASSERT_THROWS(sor(A, shorter, x), cusp::invalid_input_exception);
    cusp::csr_matrix<int, double, Space> rect(cusp::csr_matrix<int, double, cusp::host_memory>(2, 3, 0));
    ASSERT_THROWS((cusp::relaxation::gauss_seidel<double, Space>(rect)), cusp::invalid_input_exception);
    // default-constructed and empty objects
    cusp::relaxation::gauss_seidel<double, Space> none;
    cusp::relaxation::sor<double, Space> none_sor;
    ASSERT_EQUAL(none.ordering.size(), (size_t)0);
    cusp::csr_matrix<int, double, Space> E(0, 0, 0);
    cusp::array1d<double, Space> e;
    cusp::relaxation::gauss_seidel<double, Space> empty(E);
    empty(E, e, e);
    ASSERT_EQUAL(e.size(), (size_t)0);
}

} // namespace gs_check
