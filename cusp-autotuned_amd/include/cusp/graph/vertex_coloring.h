// cusp/graph/vertex_coloring.h -- size_t cusp::graph::vertex_coloring(G, colors): a greedy colouring of the graph whose
// adjacency structure is the square matrix G; returns the number of colours (reference cusp/graph/vertex_coloring.h and
// its sequential rule, system/detail/sequential/graph/vertex_coloring.h).
//
// The rule: colors starts as N - 1 everywhere; the vertices are taken in index order; a vertex marks the colours its own
// row's columns hold at that moment, takes the lowest unmarked colour below the current maximum, and opens a new colour
// when there is none.  Only row i's OWN entries are looked at: on a pattern that is not symmetric a row may hold a column
// of its own colour -- always one with a larger index, coloured later (cusp/relaxation/gauss_seidel.h handles that).
//
// Set-up work, done on the host in either memory space (the reference's device version copies to the host as well): the
// structure is read from a host CSR copy of G -- any format, through the conversions of cusp/convert.h -- and the colours
// are copied back into `colors`, which is resized to N.
#pragma once
#include <limits>
#include <vector>

#include "../array1d.h"
#include "../convert.h"
#include "../exception.h"

namespace cusp {
namespace graph {

template <typename MatrixType, typename ArrayType> size_t vertex_coloring(const MatrixType &G, ArrayType &colors)
{
    typedef typename MatrixType::index_type I;
    typedef typename ArrayType::value_type C;
    if (G.num_rows != G.num_cols) throw cusp::invalid_input_exception("cusp::graph::vertex_coloring: matrix must be square");
    cusp::detail::host_csr<I, typename MatrixType::value_type> H;
    cusp::detail::to_host_csr(G, H, typename MatrixType::format());

    const size_t N = G.num_rows;
    size_t max_color = 0;
    cusp::array1d<C, cusp::host_memory> c(N, static_cast<C>(N - 1));
    std::vector<size_t> mark(N, std::numeric_limits<size_t>::max()); // mark[colour] = the last vertex that saw it on a neighbour
    for (size_t vertex = 0; vertex < N; vertex++) {
        for (I jj = H.row_offsets[vertex]; jj < H.row_offsets[vertex + 1]; jj++) mark[static_cast<size_t>(c[H.column_indices[jj]])] = vertex;
        size_t vertex_color = 0;
        while (vertex_color < max_color && mark[vertex_color] == vertex) vertex_color++;
        if (vertex_color == max_color) max_color++;
        c[vertex] = static_cast<C>(vertex_color);
    }
    colors = c;
    return max_color;
}

// the reference's overload with an execution policy in front
template <typename Policy, typename MatrixType, typename ArrayType>
auto vertex_coloring(const Policy &, const MatrixType &G, ArrayType &colors) -> decltype(typename MatrixType::format(), size_t())
{
    return vertex_coloring(G, colors);
}

} // namespace graph
} // namespace cusp
