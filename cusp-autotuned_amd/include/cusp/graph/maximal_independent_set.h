// cusp/graph/maximal_independent_set.h -- size_t cusp::graph::maximal_independent_set(G, stencil, k = 1): a maximal
// independent set of the graph whose edges are the stored entries of the square matrix G, distance k: no two nodes of the set
// lie within k steps of each other, and every other node lies within k steps of one.  stencil[i] = 1 for the nodes of the
// set, 0 for the others (resized to N); the set's size is returned.  (reference cusp/graph/maximal_independent_set.h; its
// parallel algorithm, system/detail/generic/graph/maximal_independent_set.h.)
//
// The algorithm (include/cusp_mi355x.h states it as loops).  A node is undecided (1), in the set (2) or out (0); all start
// undecided.  A round: every node forms the key  state << 62 | r(i) << 31 | i;  k sweeps replace each key by the maximum
// over the node itself and its row's columns, each sweep reading the one before it; an undecided node whose final key carries
// its own index joins the set; then an undecided node whose final key names a node that is now in the set leaves.  Rounds
// repeat until nobody is undecided.  k = 0: every node, no sweep.  The index in the key excludes ties.
//
// Every stored entry is an edge, whatever its value; columns may repeat, rows may be unsorted, and a node sees itself
// whether or not its diagonal is stored.  The set is independent and maximal when the pattern is symmetric: the reference's
// precondition, not checked.  The rounds end on any pattern.
//
// Deviations from the reference:
//   * the random values are this library's hash, r(i) = cusp::detail::random_hash(i, seed) >> 33 (31 bits, seed 0), not the
//     reference's: the SET differs from the reference's, its properties do not;
//   * ONE algorithm in both memory spaces.  The reference's host_memory path is another algorithm (sequential and greedy);
//     here host_memory runs the parallel algorithm above as plain loops, so that host and device give the same stencil,
//     which is this library's contract.
//   host_memory   : the loops below, on a host CSR copy of G for the other formats.
//   device_memory : cmi_csr_maximal_independent_set on G's device arrays (other formats are converted to CSR first); one host
//                   read per round, no host copy of the structure.
// A column outside the matrix throws cusp::invalid_input_exception in both spaces.
#pragma once
#include <cstdint>
#include <vector>

#include "../array1d.h"
#include "../convert.h"
#include "../csr_matrix.h"
#include "../detail/random_hash.h"
#include "../exception.h"
#include "../execution_policy.h"

namespace cusp {
namespace graph {
namespace detail {

// z[i] = max(x[i], max over row i of x[column]): cmi_csr_ring_max_u64 as a loop
template <typename Csr> void ring_max(const Csr &G, const std::vector<uint64_t> &x, std::vector<uint64_t> &z)
{
    const size_t n = G.num_rows;
    z.resize(n);
    for (size_t i = 0; i < n; i++) {
        uint64_t best = x[i];
        for (auto jj = G.row_offsets[i]; jj < G.row_offsets[i + 1]; jj++) {
            const auto j = G.column_indices[jj];
            if (j < 0 || static_cast<size_t>(j) >= n) throw cusp::invalid_input_exception("maximal independent set: a column index lies outside [0, num_rows)");
            if (x[j] > best) best = x[j];
        }
        z[i] = best;
    }
}

// MIS(k), k >= 1, of a host CSR pattern: flag[i] = 1 / 0; returns the set's size
template <typename Csr> size_t mis_host(const Csr &G, std::vector<int> &flag, size_t k, uint64_t seed, size_t *rounds)
{
    const size_t n = G.num_rows;
    const uint64_t index_mask = 0x7FFFFFFFull;
    std::vector<int> state(n, 1);
    std::vector<uint64_t> x(n), y, z;
    size_t undecided = n, in_set = 0;
    *rounds = 0;
    while (undecided > 0) {
        for (size_t i = 0; i < n; i++)
            x[i] = (static_cast<uint64_t>(state[i]) << 62) | ((cusp::detail::random_hash(i, seed) >> 33) << 31) | static_cast<uint64_t>(i);
        ring_max(G, x, z);
        for (size_t ring = 1; ring < k; ring++) {
            y.swap(z);
            ring_max(G, y, z);
        }
        for (size_t i = 0; i < n; i++)
            if (state[i] == 1 && (z[i] & index_mask) == i) state[i] = 2;
        for (size_t i = 0; i < n; i++)
            if (state[i] == 1 && state[z[i] & index_mask] == 2) state[i] = 0;
        undecided = in_set = 0;
        for (size_t i = 0; i < n; i++) {
            undecided += state[i] == 1;
            in_set += state[i] == 2;
        }
        ++*rounds;
    }
    flag.resize(n);
    for (size_t i = 0; i < n; i++) flag[i] = state[i] == 2;
    return in_set;
}

template <typename Csr, typename ArrayType> size_t mis(const Csr &G, ArrayType &stencil, size_t k, uint64_t seed, size_t *rounds, cusp::host_memory)
{
    std::vector<int> flag;
    const size_t count = mis_host(G, flag, k, seed, rounds);
    stencil = cusp::array1d<int, cusp::host_memory>(flag);
    return count;
}
template <typename Csr, typename ArrayType> size_t mis(const Csr &G, ArrayType &stencil, size_t k, uint64_t seed, size_t *rounds, cusp::device_memory)
{
    static_assert(sizeof(typename Csr::index_type) == 4, "the device path takes 32-bit indices");
    cusp::array1d<int, cusp::device_memory> flag(G.num_rows);
    int64_t count = 0;
    int r = 0;
    if (k > 0x7FFFFFFFull) throw cusp::invalid_input_exception("maximal_independent_set: k is too large");
    cusp::detail::check(cmi_csr_maximal_independent_set((int64_t)G.num_rows, (int64_t)G.num_entries, G.row_offsets.data(), G.column_indices.data(), (int)k, seed,
                                                        flag.data(), &count, &r, nullptr));
    stencil = flag;
    *rounds = static_cast<size_t>(r);
    return static_cast<size_t>(count);
}

// f(G as a CSR matrix in its own memory space): G itself when it is one, a converted copy otherwise
template <typename MatrixType, typename F> auto with_csr(const MatrixType &G, F &&f, cusp::csr_format) -> decltype(f(G)) { return f(G); }
template <typename MatrixType, typename F, typename Format>
auto with_csr(const MatrixType &G, F &&f, Format) -> decltype(f(cusp::csr_matrix<typename MatrixType::index_type, typename MatrixType::value_type, typename MatrixType::memory_space>()))
{
    const cusp::csr_matrix<typename MatrixType::index_type, typename MatrixType::value_type, typename MatrixType::memory_space> csr(G);
    return f(csr);
}

// the form that takes the seed and reports the rounds
template <typename MatrixType, typename ArrayType> size_t maximal_independent_set(const MatrixType &G, ArrayType &stencil, size_t k, uint64_t seed, size_t *rounds = nullptr)
{
    if (G.num_rows != G.num_cols) throw cusp::invalid_input_exception("cusp::graph::maximal_independent_set: matrix must be square");
    size_t r = 0;
    size_t count = G.num_rows;
    if (k == 0) stencil = cusp::array1d<int, cusp::host_memory>(G.num_rows, 1); // every node, no sweep
    else count = with_csr(G, [&](const auto &csr) { return mis(csr, stencil, k, seed, &r, typename MatrixType::memory_space()); }, typename MatrixType::format());
    if (rounds) *rounds = r;
    return count;
}

} // namespace detail

template <typename MatrixType, typename ArrayType> size_t maximal_independent_set(const MatrixType &G, ArrayType &stencil, const size_t k = 1)
{
    return detail::maximal_independent_set(G, stencil, k, 0);
}

// the reference's overload with an execution policy in front
template <typename Derived, typename MatrixType, typename ArrayType>
size_t maximal_independent_set(const cusp::execution_policy<Derived> &, const MatrixType &G, ArrayType &stencil, const size_t k = 1)
{
    return detail::maximal_independent_set(G, stencil, k, 0);
}

} // namespace graph
} // namespace cusp
