// cusp/graph/pseudo_peripheral.h -- index_type cusp::graph::pseudo_peripheral_vertex(G [, levels]): a vertex far from the rest
// of the graph, found by repeated searches (reference cusp/graph/pseudo_peripheral.h; its loop,
// system/detail/generic/graph/pseudo_peripheral.h):
//     x = start; delta = 0
//     repeat: levels = the levels of the search from x; y = the vertex of the last level with the smallest row length, the
//             smallest index among equals; if levels[y] <= delta: return y; x = y; delta = levels[y]
// levels (resized to N) holds the levels of the last search that ran.  A matrix without entries: every level is -1 and the
// answer is vertex 0.
//
// Deviations from the reference:
//   * the first vertex is 0 (the reference draws rand() % N); detail::pseudo_peripheral_vertex takes `start`;
//   * the row lengths compared are those of the last-level vertices themselves.  The reference gathers row_lengths[0 .. count),
//     the lengths of the first `count` vertices of the graph: a bug.
//   host_memory   : the loop below on detail::bfs_host.
//   device_memory : cmi_csr_pseudo_peripheral_vertex (y is one integer reduction on the device).
// Refusals as in breadth_first_search.h, cusp::invalid_input_exception in both spaces.
#pragma once
#include "breadth_first_search.h"

namespace cusp {
namespace graph {
namespace detail {

template <typename Csr> int64_t peripheral(const Csr &G, int64_t start, cusp::array1d<int, cusp::host_memory> &levels, int *searches, cusp::host_memory)
{
    const int64_t n = (int64_t)G.num_rows, nnz = (int64_t)G.num_entries;
    const auto clamp = [nnz](int64_t p) { return p < 0 ? (int64_t)0 : (p > nnz ? nnz : p); };
    std::vector<int> level;
    int64_t x = start;
    int delta = 0;
    for (*searches = 1;; ++*searches) {
        size_t reached = 0;
        int depth = -1;
        bfs_host(G, x, true, level, &reached, &depth);
        int64_t y = -1, best = 0;
        for (int64_t v = 0; v < n; v++) {
            if (level[v] != depth) continue;
            const int64_t lo = clamp(G.row_offsets[v]), hi = clamp(G.row_offsets[v + 1]), length = hi > lo ? hi - lo : 0;
            if (y < 0 || length < best) { y = v; best = length; }
        }
        if (depth <= delta) { // (level[y] == depth)
            levels = cusp::array1d<int, cusp::host_memory>(level);
            return y;
        }
        x = y;
        delta = depth;
    }
}
template <typename Csr> int64_t peripheral(const Csr &G, int64_t start, cusp::array1d<int, cusp::device_memory> &levels, int *searches, cusp::device_memory)
{
    static_assert(sizeof(typename Csr::index_type) == 4, "the device path takes 32-bit indices");
    cusp::array1d<int, cusp::device_memory> out(G.num_rows);
    int64_t vertex = 0;
    cusp::detail::check(cmi_csr_pseudo_peripheral_vertex((int64_t)G.num_rows, (int64_t)G.num_entries, G.row_offsets.data(), G.column_indices.data(), start, out.data(),
                                                         &vertex, searches, nullptr));
    levels.swap(out);
    return vertex;
}

// the form that takes the first vertex and reports the number of searches; levels in the matrix's memory space
template <typename MatrixType>
typename MatrixType::index_type pseudo_peripheral_vertex(const MatrixType &G, cusp::array1d<int, typename MatrixType::memory_space> &levels, int64_t start,
                                                         int *searches = nullptr)
{
    require_square(G.num_rows, G.num_cols, "cusp::graph::pseudo_peripheral_vertex");
    int count = 0;
    const int64_t y = with_csr(G, [&](const auto &csr) { return peripheral(csr, start, levels, &count, typename MatrixType::memory_space()); }, typename MatrixType::format());
    if (searches) *searches = count;
    return (typename MatrixType::index_type)y;
}

} // namespace detail

template <typename MatrixType, typename ArrayType> typename MatrixType::index_type pseudo_peripheral_vertex(const MatrixType &G, ArrayType &levels)
{
    cusp::array1d<int, typename MatrixType::memory_space> out;
    const typename MatrixType::index_type y = detail::pseudo_peripheral_vertex(G, out, 0);
    levels = out;
    return y;
}
template <typename MatrixType> typename MatrixType::index_type pseudo_peripheral_vertex(const MatrixType &G)
{
    cusp::array1d<int, typename MatrixType::memory_space> levels;
    return detail::pseudo_peripheral_vertex(G, levels, 0);
}

// the reference's overloads with an execution policy in front
template <typename Derived, typename MatrixType, typename ArrayType>
typename MatrixType::index_type pseudo_peripheral_vertex(const cusp::execution_policy<Derived> &, const MatrixType &G, ArrayType &levels)
{
    return cusp::graph::pseudo_peripheral_vertex(G, levels);
}
template <typename Derived, typename MatrixType>
typename MatrixType::index_type pseudo_peripheral_vertex(const cusp::execution_policy<Derived> &, const MatrixType &G)
{
    return cusp::graph::pseudo_peripheral_vertex(G);
}

} // namespace graph
} // namespace cusp
