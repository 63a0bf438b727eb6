// cusp/graph/connected_components.h -- size_t cusp::graph::connected_components(G, components): components[i] = the number of
// the component of vertex i (resized to N), the count returned (reference cusp/graph/connected_components.h; its loop over
// searches, system/detail/generic/graph/connected_components.h):
//     count = 0; src = 0
//     repeat: search from src; every vertex the search reaches gets `count` -- one already numbered too, as in the reference;
//             count += 1; src = the first vertex without a number, stop when there is none
// The search follows rows (breadth_first_search.h), so on a pattern that is not symmetric the numbers depend on the direction
// of the edges: the reference's precondition is a symmetric pattern.
//
// Deviations from the reference: the first source is 0 (the reference draws rand() % N), and src itself always receives the
// number -- on a matrix without entries a search reaches nobody, and the reference loops forever.
// One search per component in both memory spaces (device_memory: cmi_csr_breadth_first_search per search, its labels read
// back by the host); a hook-and-shortcut kernel would need one pass, and is not here.
#pragma once
#include "breadth_first_search.h"

namespace cusp {
namespace graph {

template <typename MatrixType, typename ArrayType> size_t connected_components(const MatrixType &G, ArrayType &components)
{
    typedef typename MatrixType::memory_space Space;
    detail::require_square(G.num_rows, G.num_cols, "cusp::graph::connected_components");
    const size_t n = G.num_rows;
    std::vector<int> number(n, -1);
    size_t count = 0;
    detail::with_csr(G, [&](const auto &csr) {
        cusp::array1d<int, Space> labels;
        for (size_t src = 0; src < n;) {
            size_t reached = 0;
            int depth = -1;
            detail::bfs(csr, (int64_t)src, true, labels, &reached, &depth, Space());
            const auto &level = cusp::detail::host_copy(labels);
            for (size_t i = 0; i < n; i++)
                if (level[i] >= 0) number[i] = (int)count;
            number[src] = (int)count;
            count++;
            while (src < n && number[src] != -1) src++;
        }
        return 0;
    }, typename MatrixType::format());
    components = cusp::array1d<int, cusp::host_memory>(number);
    return count;
}

// the reference's overload with an execution policy in front
template <typename Derived, typename MatrixType, typename ArrayType>
size_t connected_components(const cusp::execution_policy<Derived> &, const MatrixType &G, ArrayType &components)
{
    return cusp::graph::connected_components(G, components);
}

} // namespace graph
} // namespace cusp
