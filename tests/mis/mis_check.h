// Shared by the MIS test programs: the graphs, results gathered per format and memory space, and the set-up of
// smoothed_aggregation::extend_hierarchy with mis_aggregate and the caller's rho per level (amg_check::build with the other
// aggregation), so that hierarchies can be compared bit for bit between memory spaces.
#pragma once
#include "amg_check.h"

#include <cusp/dia_matrix.h>
#include <cusp/graph/maximal_independent_set.h>
#include <cusp/hyb_matrix.h>

namespace mis_check {

using namespace amg_check;

// a pattern from rows of columns, every value 1
inline host_csr<double> pattern(const std::vector<std::vector<int>> &rows)
{
    size_t nnz = 0;
    for (auto &r : rows) nnz += r.size();
    host_csr<double> A(rows.size(), rows.size(), nnz);
    size_t at = 0;
    for (size_t i = 0; i < rows.size(); i++) {
        A.row_offsets[i] = (int)at;
        for (int j : rows[i]) { A.column_indices[at] = j; A.values[at] = 1.0; at++; }
    }
    A.row_offsets[rows.size()] = (int)at;
    return A;
}
inline host_csr<double> poisson(size_t nx, size_t ny)
{
    host_csr<double> A;
    cusp::gallery::poisson5pt(A, nx, ny);
    return A;
}
// the graphs of the reference's test (explicit zeros removed)
inline std::vector<std::pair<std::string, host_csr<double>>> reference_graphs()
{
    std::vector<std::pair<std::string, host_csr<double>>> out;
    out.push_back({"two components of two", pattern({{0, 1}, {0, 1}, {2, 3}, {2, 3}})});
    out.push_back({"path of 4", pattern({{0, 1}, {0, 1, 2}, {1, 2, 3}, {2, 3}})});
    out.push_back({"K6", pattern(std::vector<std::vector<int>>(6, {0, 1, 2, 3, 4, 5}))});
    out.push_back({"six isolated", pattern(std::vector<std::vector<int>>(6))});
    out.push_back({"poisson 3x3", poisson(3, 3)});
    out.push_back({"poisson 13x17", poisson(13, 17)});
    out.push_back({"poisson 23x24", poisson(23, 24)});
    out.push_back({"poisson 105x107", poisson(105, 107)});
    return out;
}

struct result {
    std::vector<int> stencil[4], aggregates, mis; // stencil[k], k = 0..3
    size_t size[4], rounds[4];
    bool operator==(const result &o) const
    {
        for (int k = 0; k < 4; k++)
            if (stencil[k] != o.stencil[k] || size[k] != o.size[k] || rounds[k] != o.rounds[k]) return false;
        return aggregates == o.aggregates && mis == o.mis;
    }
};
template <typename Matrix> result run(const Matrix &G, uint64_t seed)
{
    typedef typename Matrix::memory_space Space;
    result r;
    for (int k = 0; k < 4; k++) {
        cusp::array1d<int, Space> stencil;
        r.size[k] = cusp::graph::detail::maximal_independent_set(G, stencil, (size_t)k, seed, &r.rounds[k]);
        r.stencil[k] = cusp::detail::host_copy(stencil);
    }
    cusp::array1d<int, Space> aggregates, mis;
    agg::detail::mis_aggregate(G, aggregates, mis, seed);
    r.aggregates = cusp::detail::host_copy(aggregates);
    r.mis = cusp::detail::host_copy(mis);
    return r;
}
// the five formats of one memory space, each against `want`
template <typename Space> bool five_formats_give(const host_csr<double> &A, uint64_t seed, const result &want)
{
    bool ok = run(cusp::csr_matrix<int, double, Space>(A), seed) == want;
    ok = run(cusp::coo_matrix<int, double, Space>(A), seed) == want && ok;
    ok = run(cusp::ell_matrix<int, double, Space>(A), seed) == want && ok;
    ok = run(cusp::dia_matrix<int, double, Space>(A), seed) == want && ok;
    ok = run(cusp::hyb_matrix<int, double, Space>(A), seed) == want && ok;
    return ok;
}

template <typename V, typename Space, typename Matrix> std::vector<built_level<V, Space>> build_mis(const Matrix &A0, const std::vector<double> &rhos, size_t min_level_size)
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
            agg::symmetric_strength_of_connection(L.A, L.S, 0.0);
            agg::mis_aggregate(L.S, L.aggregates);
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

} // namespace mis_check
