// Shared by the AMG test programs: a hierarchy built from the components with the caller's rho per level (so that values can
// be compared bit for bit between memory spaces and against tests/amg_refs.py), bitwise comparisons, and the cg counts.
#pragma once
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include <cusp/coo_matrix.h>
#include <cusp/csr_matrix.h>
#include <cusp/ell_matrix.h>
#include <cusp/elementwise.h>
#include <cusp/gallery/poisson.h>
#include <cusp/io/matrix_market.h>
#include <cusp/krylov/cg.h>
#include <cusp/monitor.h>
#include <cusp/precond/aggregation/smoothed_aggregation.h>

#include "unittest.h"

namespace amg_check {

namespace agg = cusp::precond::aggregation;
template <typename V> using host_csr = cusp::csr_matrix<int, V, cusp::host_memory>;

template <typename V, typename Space> struct built_level {
    cusp::csr_matrix<int, V, Space> A, S, T, P, R;
    cusp::array1d<int, Space> aggregates;
    cusp::array1d<V, Space> B;
};

// the set-up of smoothed_aggregation::extend_hierarchy with rho supplied; the last element holds the coarsest A and B only
template <typename V, typename Space, typename Matrix> std::vector<built_level<V, Space>> build(const Matrix &A0, const std::vector<double> &rhos, size_t min_level_size, double theta = 0.0)
{
    std::vector<built_level<V, Space>> out(1);
    out[0].A = A0;
    out[0].B = cusp::array1d<V, Space>(A0.num_rows, V(1));
    while (out.back().A.num_rows > min_level_size && out.size() <= rhos.size()) {
        const double rho = rhos[out.size() - 1];
        cusp::csr_matrix<int, V, Space> RAP;
        cusp::array1d<V, Space> Bc;
        {
            built_level<V, Space> &L = out.back();
            agg::symmetric_strength_of_connection(L.A, L.S, theta);
            agg::standard_aggregate(L.S, L.aggregates);
            agg::fit_candidates(L.aggregates, L.B, L.T, Bc);
            agg::smooth_prolongator(L.A, L.T, L.P, rho);
            agg::form_restriction(L.P, L.R);
            agg::galerkin_product(L.R, L.A, L.P, RAP);
        }
        out.emplace_back();
        out.back().A.swap(RAP);
        out.back().B = Bc;
    }
    return out;
}

template <typename V> bool bits_equal(const std::vector<V> &a, const std::vector<V> &b)
{
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(V)) == 0);
}
template <typename A, typename B> bool arrays_bits_equal(const A &a, const B &b) { return bits_equal(cusp::detail::host_copy(a), cusp::detail::host_copy(b)); }
template <typename MA, typename MB> bool csr_bits_equal(const MA &a, const MB &b)
{
    return a.num_rows == b.num_rows && a.num_cols == b.num_cols && a.num_entries == b.num_entries && arrays_bits_equal(a.row_offsets, b.row_offsets) &&
           arrays_bits_equal(a.column_indices, b.column_indices) && arrays_bits_equal(a.values, b.values);
}
// a with its entries that compare equal to zero removed (what the host product drops and the device product keeps)
template <typename V, typename M> host_csr<V> without_zeros(const M &m)
{
    host_csr<V> h(m), out(h.num_rows, h.num_cols, 0);
    std::vector<int> cj;
    std::vector<V> cx;
    for (size_t i = 0; i < h.num_rows; i++) {
        out.row_offsets[i] = (int)cj.size();
        for (int q = h.row_offsets[i]; q < h.row_offsets[i + 1]; q++)
            if (!(h.values[q] == V(0))) {
                cj.push_back(h.column_indices[q]);
                cx.push_back(h.values[q]);
            }
    }
    out.resize(h.num_rows, h.num_cols, cj.size());
    size_t at = 0;
    for (size_t i = 0; i < h.num_rows; i++) {
        out.row_offsets[i] = (int)at;
        for (int q = h.row_offsets[i]; q < h.row_offsets[i + 1]; q++)
            if (!(h.values[q] == V(0))) {
                out.column_indices[at] = h.column_indices[q];
                out.values[at] = h.values[q];
                at++;
            }
    }
    out.row_offsets[h.num_rows] = (int)at;
    return out;
}

// An irregular square matrix: 0..max_len entries per row anywhere (pattern not symmetric, columns sorted, a column may repeat), no diagonal in
// every seventh row, empty rows, rows holding their diagonal alone (isolated nodes), values small multiples of 1/4 so that sums cancel exactly
template <typename V> host_csr<V> irregular_square(size_t n, int max_len, uint64_t salt, bool missing_diagonals = true)
{
    auto mix = [](uint64_t i) { uint64_t z = i * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull; z ^= z >> 31; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 29; return z; };
    std::vector<std::vector<std::pair<int, V>>> rows(n);
    size_t nnz = 0;
    for (size_t i = 0; i < n; i++) {
        const int len = (int)(mix(salt + i) % (uint64_t)(max_len + 1));
        if (i % 11 == 5) rows[i].push_back({(int)i, V(2)});                  // isolated: the diagonal alone
        else
            for (int t = 0; t < len; t++) {
                const uint64_t h = salt + 977 * i + 13 * (uint64_t)t;
                const long span = 40;                                          // neighbours within +-40: aggregates of several rows form
                long c = (long)i + (long)(mix(h) % (2 * span + 1)) - span;
                c = c < 0 ? 0 : (c >= (long)n ? (long)n - 1 : c);
                rows[i].push_back({(int)c, V((double)((long)(mix(h + 5) % 17) - 8) * 0.25)});
            }
        if ((i % 7 != 3 || !missing_diagonals) && i % 11 != 5 && len > 0) rows[i].push_back({(int)i, V(4)});
        std::stable_sort(rows[i].begin(), rows[i].end(), [](const std::pair<int, V> &x, const std::pair<int, V> &y) { return x.first < y.first; });
        nnz += rows[i].size();
    }
    host_csr<V> A(n, n, nnz);
    size_t at = 0;
    for (size_t i = 0; i < n; i++) {
        A.row_offsets[i] = (int)at;
        for (auto &e : rows[i]) { A.column_indices[at] = e.first; A.values[at] = e.second; at++; }
    }
    A.row_offsets[n] = (int)at;
    return A;
}

// entries of the product A B that exist structurally: what a product that keeps exact-zero sums holds
template <typename V> size_t structural_product_entries(const host_csr<V> &A, const host_csr<V> &B)
{
    host_csr<V> a(A), b(B), c;
    for (size_t q = 0; q < a.num_entries; q++) a.values[q] = V(1);
    for (size_t q = 0; q < b.num_entries; q++) b.values[q] = V(1);
    cusp::multiply(a, b, c);
    return c.num_entries;
}

// b[i] from a fixed hash in [-1, 1)
template <typename V, typename Space> cusp::array1d<V, Space> seeded_rhs(size_t n)
{
    cusp::array1d<V, cusp::host_memory> b(n);
    for (size_t i = 0; i < n; i++) {
        uint64_t z = (i + 1) * 0x9E3779B97F4A7C15ull;
        z ^= z >> 31; z *= 0xBF58476D1CE4E5B9ull; z ^= z >> 29;
        b[i] = V((double)(z % 65536) / 32768.0 - 1.0);
    }
    return cusp::array1d<V, Space>(b);
}

// iterations of cg to a relative residual of 1e-8 (0 preconditioner: none); -1 when it did not converge in 2000
template <typename Matrix, typename Vector, typename Precond> long cg_count(const Matrix &A, const Vector &b, const Precond *M)
{
    typedef typename Matrix::value_type V;
    Vector x(A.num_rows, V(0));
    cusp::monitor<V> monitor(b, 2000, 1e-8);
    if (M) cusp::krylov::cg(A, x, b, monitor, *M);
    else cusp::krylov::cg(A, x, b, monitor);
    return monitor.converged() ? (long)monitor.iteration_count() : -1;
}

} // namespace amg_check
