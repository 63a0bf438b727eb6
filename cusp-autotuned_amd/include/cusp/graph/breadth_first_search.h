// cusp/graph/breadth_first_search.h -- void cusp::graph::breadth_first_search(G, src, labels, mark_levels = true): the search
// from vertex src of the graph whose edges are the stored entries of the square matrix G (reference
// cusp/graph/breadth_first_search.h; its host loop, system/detail/sequential/graph/breadth_first_search.h).
//
// Every stored entry of row u is an edge u -> column, whatever its value; columns may repeat, rows may be unsorted.  Edges are
// DIRECTED: the search follows rows.  A column of -1 is skipped, as in the reference's loop.  labels is resized to N:
//   mark_levels     labels[i] = the level of i (src: 0), -1 for a vertex the search does not reach
//   !mark_levels    labels[i] = a predecessor of i; -2 for src, -1 for a vertex not reached
// A matrix without entries leaves every label at -1 (the reference's host behaviour).
//
// Deviation from the reference: the predecessor is THE SMALLEST-NUMBERED VERTEX OF THE PREVIOUS LEVEL THAT HAS AN EDGE TO i,
// in both memory spaces (one algorithm everywhere, as for maximal_independent_set).  The reference's host loop records the
// first discoverer in queue order, and its device path whichever thread wins.
//   host_memory   : the loop below (the contract of include/cusp_mi355x.h), on a host CSR copy of G for the other formats.
//   device_memory : cmi_csr_breadth_first_search on G's device arrays (other formats are converted to CSR first).
// A matrix that is not square, a source outside [0, N), and a column other than -1 outside the matrix in a row the search
// reaches throw cusp::invalid_input_exception in both spaces; labels is then left as it was.
#pragma once
#include <climits>
#include <cstdint>
#include <vector>

#include "maximal_independent_set.h" // detail::with_csr

namespace cusp {
namespace graph {
namespace detail {

// cmi_csr_breadth_first_search as a loop: levels (and the smallest discoverers) of a host CSR pattern
template <typename Csr> void bfs_host(const Csr &G, int64_t src, bool mark_levels, std::vector<int> &labels, size_t *reached, int *depth)
{
    const int64_t n = (int64_t)G.num_rows, nnz = (int64_t)G.num_entries;
    if (src < 0 || src >= n) throw cusp::invalid_input_exception("breadth-first search: the source vertex lies outside [0, num_rows)");
    *reached = 0;
    *depth = -1;
    if (nnz == 0) {
        labels.assign((size_t)n, -1);
        return;
    }
    const auto clamp = [nnz](int64_t p) { return p < 0 ? (int64_t)0 : (p > nnz ? nnz : p); };
    std::vector<int> level((size_t)n, -1), pred(mark_levels ? (size_t)0 : (size_t)n, INT_MAX), frontier(1, (int)src), next;
    level[(size_t)src] = 0;
    int d = 0;
    size_t count = 1;
    while (!frontier.empty()) {
        next.clear();
        for (const int u : frontier)
            for (int64_t jj = clamp(G.row_offsets[u]); jj < clamp(G.row_offsets[u + 1]); jj++) {
                const int64_t j = G.column_indices[jj];
                if (j == -1) continue;
                if (j < 0 || j >= n) throw cusp::invalid_input_exception("breadth-first search: a column index lies outside [0, num_rows)");
                if (level[j] == -1) {
                    level[j] = d + 1;
                    next.push_back((int)j);
                }
                if (!mark_levels && level[j] == d + 1 && u < pred[j]) pred[j] = u;
            }
        if (!next.empty()) d++;
        count += next.size();
        frontier.swap(next);
    }
    if (!mark_levels)
        for (int64_t i = 0; i < n; i++) level[i] = level[i] < 0 ? -1 : (i == src ? -2 : pred[i]);
    labels.swap(level);
    *reached = count;
    *depth = d;
}

template <typename Csr> void bfs(const Csr &G, int64_t src, bool mark_levels, cusp::array1d<int, cusp::host_memory> &labels, size_t *reached, int *depth, cusp::host_memory)
{
    std::vector<int> out;
    bfs_host(G, src, mark_levels, out, reached, depth);
    labels = cusp::array1d<int, cusp::host_memory>(out);
}
template <typename Csr> void bfs(const Csr &G, int64_t src, bool mark_levels, cusp::array1d<int, cusp::device_memory> &labels, size_t *reached, int *depth, cusp::device_memory)
{
    static_assert(sizeof(typename Csr::index_type) == 4, "the device path takes 32-bit indices");
    cusp::array1d<int, cusp::device_memory> out(G.num_rows);
    int64_t count = 0;
    cusp::detail::check(cmi_csr_breadth_first_search((int64_t)G.num_rows, (int64_t)G.num_entries, G.row_offsets.data(), G.column_indices.data(), src, mark_levels ? 1 : 0,
                                                     out.data(), &count, depth, nullptr));
    labels.swap(out);
    *reached = (size_t)count;
}

inline void require_square(size_t rows, size_t cols, const char *who)
{
    if (rows != cols) throw cusp::invalid_input_exception(std::string(who) + ": matrix must be square");
}

// the form that reports how many vertices were reached and the deepest level; labels in the matrix's memory space
template <typename MatrixType>
void breadth_first_search(const MatrixType &G, int64_t src, cusp::array1d<int, typename MatrixType::memory_space> &labels, bool mark_levels, size_t *reached, int *depth)
{
    require_square(G.num_rows, G.num_cols, "cusp::graph::breadth_first_search");
    with_csr(G, [&](const auto &csr) { bfs(csr, src, mark_levels, labels, reached, depth, typename MatrixType::memory_space()); return 0; }, typename MatrixType::format());
}

} // namespace detail

template <typename MatrixType, typename ArrayType>
void breadth_first_search(const MatrixType &G, const typename MatrixType::index_type src, ArrayType &labels, const bool mark_levels = true)
{
    cusp::array1d<int, typename MatrixType::memory_space> out;
    size_t reached = 0;
    int depth = -1;
    detail::breadth_first_search(G, (int64_t)src, out, mark_levels, &reached, &depth);
    labels = out;
}

// the reference's overload with an execution policy in front
template <typename Derived, typename MatrixType, typename ArrayType>
void breadth_first_search(const cusp::execution_policy<Derived> &, const MatrixType &G, const typename MatrixType::index_type src, ArrayType &labels,
                          const bool mark_levels = true)
{
    cusp::graph::breadth_first_search(G, src, labels, mark_levels);
}

} // namespace graph
} // namespace cusp
