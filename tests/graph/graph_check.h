// Shared by the graph test programs: everything the graph headers compute for one matrix, gathered on the host so that formats
// and memory spaces can be compared entry for entry.
#pragma once
#include "mis_check.h"

#include <cusp/graph/breadth_first_search.h>
#include <cusp/graph/connected_components.h>
#include <cusp/graph/pseudo_peripheral.h>
#include <cusp/graph/symmetric_rcm.h>
#include <cusp/multiply.h>
#include <cusp/permutation_matrix.h>

namespace graph_check {

using amg_check::host_csr;
using mis_check::pattern;
using mis_check::poisson;
using mis_check::reference_graphs;

struct result {
    std::vector<int> levels, preds, last_levels, permutation, components, rows, cols;
    std::vector<double> values, gathered, scattered;
    size_t reached = 0, count = 0;
    int depth = -1, searches = 0;
    long vertex = -1, rcm_vertex = -1;
    bool permuted = false; // false: the format refused the permuted matrix (DIA: too many diagonals), as the reference's conversion does
    bool operator==(const result &o) const
    {
        return levels == o.levels && preds == o.preds && last_levels == o.last_levels && permutation == o.permutation && components == o.components &&
               (!permuted || !o.permuted || (rows == o.rows && cols == o.cols && values == o.values)) && gathered == o.gathered && scattered == o.scattered && reached == o.reached && count == o.count && depth == o.depth &&
               searches == o.searches && vertex == o.vertex && rcm_vertex == o.rcm_vertex;
    }
};

// the search from src, the pseudo-peripheral vertex and the ordering from `start`, the components, and G permuted by the ordering
template <typename Matrix> result run(const Matrix &G, long src, long start)
{
    typedef typename Matrix::memory_space Space;
    namespace gd = cusp::graph::detail;
    result r;
    cusp::array1d<int, Space> labels;
    size_t reached = 0;
    int depth = 0;
    gd::breadth_first_search(G, src, labels, false, &reached, &depth);
    r.preds = cusp::detail::host_copy(labels);
    gd::breadth_first_search(G, src, labels, true, &r.reached, &r.depth);
    r.levels = cusp::detail::host_copy(labels);
    if (reached != r.reached || depth != r.depth) r.reached = (size_t)-1; // (both forms count alike)
    r.vertex = gd::pseudo_peripheral_vertex(G, labels, start, &r.searches);
    r.last_levels = cusp::detail::host_copy(labels);
    cusp::permutation_matrix<int, Space> P;
    r.rcm_vertex = gd::symmetric_rcm(G, P, start);
    r.permutation = cusp::detail::host_copy(P.permutation);
    cusp::array1d<int, Space> components;
    r.count = cusp::graph::connected_components(G, components);
    r.components = cusp::detail::host_copy(components);
    try {
        Matrix A(G);
        P.symmetric_permute(A);
        cusp::coo_matrix<int, double, cusp::host_memory> C(A);
        C.sort_by_row_and_column();
        r.rows.assign(C.row_indices.begin(), C.row_indices.end());
        r.cols.assign(C.column_indices.begin(), C.column_indices.end());
        r.values.assign(C.values.begin(), C.values.end());
        r.permuted = true;
    } catch (const cusp::format_conversion_exception &) {
        if (!std::is_same<typename Matrix::format, cusp::dia_format>::value) throw;
    }
    std::vector<double> x(G.num_rows);
    for (size_t i = 0; i < x.size(); i++) x[i] = 0.5 + (double)i;
    const cusp::array1d<double, Space> dx(x);
    cusp::array1d<double, Space> y(G.num_rows, -1.0);
    cusp::multiply(P, dx, y);
    r.gathered = cusp::detail::host_copy(y);
    cusp::multiply(dx, P, y);
    r.scattered = cusp::detail::host_copy(y);
    return r;
}

// a copy of the pattern whose values tell the entries apart
inline host_csr<double> numbered(const host_csr<double> &A)
{
    host_csr<double> B(A);
    for (size_t e = 0; e < B.num_entries; e++) B.values[e] = 1.0 + (double)e;
    return B;
}

// the five formats of one memory space, each against `want`
template <typename Space> bool five_formats_give(const host_csr<double> &A, long src, long start, const result &want)
{
    bool ok = run(cusp::csr_matrix<int, double, Space>(A), src, start) == want;
    ok = run(cusp::coo_matrix<int, double, Space>(A), src, start) == want && ok;
    ok = run(cusp::ell_matrix<int, double, Space>(A), src, start) == want && ok;
    ok = run(cusp::dia_matrix<int, double, Space>(A), src, start) == want && ok;
    ok = run(cusp::hyb_matrix<int, double, Space>(A), src, start) == want && ok;
    return ok;
}

// the stored pattern permuted by hand: what symmetric_permute must give
inline bool permuted_by_hand(const host_csr<double> &A, const result &r)
{
    std::vector<std::pair<std::pair<int, int>, double>> e;
    for (size_t i = 0; i < A.num_rows; i++)
        for (int jj = A.row_offsets[i]; jj < A.row_offsets[i + 1]; jj++) e.push_back({{r.permutation[i], r.permutation[(size_t)A.column_indices[jj]]}, A.values[jj]});
    std::stable_sort(e.begin(), e.end(), [](const auto &a, const auto &b) { return a.first < b.first; });
    if (e.size() != r.rows.size()) return false;
    for (size_t k = 0; k < e.size(); k++)
        if (e[k].first.first != r.rows[k] || e[k].first.second != r.cols[k] || e[k].second != r.values[k]) return false;
    return true;
}

} // namespace graph_check
