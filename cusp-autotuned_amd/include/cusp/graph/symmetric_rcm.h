// cusp/graph/symmetric_rcm.h -- void cusp::graph::symmetric_rcm(G, P): a bandwidth-reducing ordering of the graph of the square
// matrix G, left in the permutation matrix P (P.permutation[v] = the new number of v; P.symmetric_permute(A) applies it).
// (reference cusp/graph/symmetric_rcm.h; system/detail/generic/graph/symmetric_rcm.h.)
//
// As in the reference: the levels of the search from a pseudo-peripheral vertex (pseudo_peripheral.h), the vertices ordered
// by (level, index) -- the reference's stable sort_by_key of the levels, so vertices the search did not reach (level -1) come
// first.  Despite the name this is a LEVEL ORDERING, not a reversed Cuthill-McKee with degree order inside the levels: the
// name and the behaviour are the reference's.  On a symmetric connected pattern no edge is longer than the widest pair of
// adjacent levels.
//   host_memory   : a counting sort of the levels below.
//   device_memory : cmi_csr_symmetric_rcm (the library's radix sort of level << 32 | index).
// The two give the same permutation.  Refusals as in breadth_first_search.h.
#pragma once
#include "pseudo_peripheral.h"
#include "../permutation_matrix.h"

namespace cusp {
namespace graph {
namespace detail {

template <typename Csr> int64_t level_order(const Csr &G, int64_t start, cusp::array1d<int, cusp::host_memory> &permutation, cusp::host_memory)
{
    cusp::array1d<int, cusp::host_memory> levels;
    int searches = 0;
    const int64_t vertex = peripheral(G, start, levels, &searches, cusp::host_memory());
    const size_t n = G.num_rows;
    int depth = -1;
    for (size_t v = 0; v < n; v++) depth = levels[v] > depth ? levels[v] : depth;
    std::vector<int> first((size_t)depth + 3, 0); // first[l + 2] counts level l, then: first[l + 1] = the position of level l's first vertex
    for (size_t v = 0; v < n; v++) first[(size_t)(levels[v] + 2)]++;
    for (size_t l = 1; l < first.size(); l++) first[l] += first[l - 1];
    permutation.resize(n);
    for (size_t v = 0; v < n; v++) permutation[v] = first[(size_t)(levels[v] + 1)]++;
    return vertex;
}
template <typename Csr> int64_t level_order(const Csr &G, int64_t start, cusp::array1d<int, cusp::device_memory> &permutation, cusp::device_memory)
{
    static_assert(sizeof(typename Csr::index_type) == 4, "the device path takes 32-bit indices");
    cusp::array1d<int, cusp::device_memory> out(G.num_rows);
    int64_t vertex = 0;
    cusp::detail::check(cmi_csr_symmetric_rcm((int64_t)G.num_rows, (int64_t)G.num_entries, G.row_offsets.data(), G.column_indices.data(), start, out.data(), &vertex, nullptr));
    permutation.swap(out);
    return vertex;
}

// the form that takes the first vertex of the pseudo-peripheral search and returns the vertex it found
template <typename MatrixType, typename PermutationType> typename MatrixType::index_type symmetric_rcm(const MatrixType &G, PermutationType &P, int64_t start)
{
    require_square(G.num_rows, G.num_cols, "cusp::graph::symmetric_rcm");
    cusp::array1d<int, typename MatrixType::memory_space> permutation;
    const int64_t vertex = with_csr(G, [&](const auto &csr) { return level_order(csr, start, permutation, typename MatrixType::memory_space()); }, typename MatrixType::format());
    P.resize(G.num_rows);
    P.permutation = permutation;
    return (typename MatrixType::index_type)vertex;
}

} // namespace detail

template <typename MatrixType, typename PermutationType> void symmetric_rcm(const MatrixType &G, PermutationType &P) { detail::symmetric_rcm(G, P, 0); }

// the reference's overload with an execution policy in front
template <typename Derived, typename MatrixType, typename PermutationType>
void symmetric_rcm(const cusp::execution_policy<Derived> &, const MatrixType &G, PermutationType &P)
{
    detail::symmetric_rcm(G, P, 0);
}

} // namespace graph
} // namespace cusp
