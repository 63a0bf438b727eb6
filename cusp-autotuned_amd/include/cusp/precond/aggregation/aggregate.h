// cusp/precond/aggregation/aggregate.h -- standard_aggregate(C, aggregates[, roots]) and aggregate(C, aggregates)
// (reference cusp/precond/aggregation/aggregate.h; system/detail/sequential/standard_aggregate.h): the three-pass sequential
// aggregation on the structure of the strength matrix C; aggregates[i] = -1 for a node without neighbours.
// Set-up work on the host in BOTH memory spaces, on a host copy of C's structure (the precedent is
// cusp::graph::vertex_coloring); the result is copied into `aggregates`' space.
//
// mis_aggregate(C, aggregates[, mis]) (reference precond/aggregation/system/detail/generic/mis_aggregate.h, the reference's
// device_memory aggregation): aggregates grown around the nodes of a distance-2 maximal independent set of C's pattern
// (cusp/graph/maximal_independent_set.h).  mis[i] = 1 for the set's nodes.  With mis = MIS(2): every node forms the key
// mis << 31 | i; one sweep takes the maximum over the node and its row; mis << 31 is added (a set node now carries 2, its
// neighbours 1, so a set node wins what follows); a second sweep; a node joins the set node its final key names, numbered by
// the exclusive prefix sums of mis.  Ids with fewer than two members are removed -- an isolated node is its own set node: the
// reference's singletons -- and their nodes get -1; the remaining ids are renumbered densely in order.
//   host_memory   : those loops.   device_memory : cmi_csr_mis_aggregate on C's device arrays, no host copy of the structure.
// Both spaces give the same arrays.  Two rules are this library's own: a node whose final key has a top part of 0 -- no set
// node within two steps -- gets -1 (the reference would gather an id from outside the range; a guard only: a node leaves the
// MIS(2) rounds on seeing a set node within two steps of its own rows, so the case does not arise with the set computed
// here); and an id left without any member, which takes a non-symmetric pattern, is removed like a singleton.
// The pattern is expected to be symmetric (the reference's precondition, not checked).  aggregate() stays standard_aggregate
// in both spaces: MIS aggregation is asked for by name, or by smoothed_aggregation::mis_aggregation.
#pragma once
#include <cstdint>
#include <vector>

#include "../../array1d.h"
#include "../../convert.h"
#include "../../exception.h"
#include "../../graph/maximal_independent_set.h"

namespace cusp {
namespace precond {
namespace aggregation {

template <typename MatrixType, typename ArrayType1, typename ArrayType2> void standard_aggregate(const MatrixType &C, ArrayType1 &aggregates, ArrayType2 &roots)
{
    typedef typename MatrixType::index_type I;
    if (C.num_rows != C.num_cols) throw cusp::invalid_input_exception("standard_aggregate: matrix must be square");
    cusp::detail::host_csr<I, typename MatrixType::value_type> H;
    cusp::detail::to_host_csr(C, H, typename MatrixType::format());
    const I n = static_cast<I>(C.num_rows);
    cusp::array1d<I, cusp::host_memory> agg(C.num_rows, I(0)), root(C.num_rows, I(0));
    I next = 1;
    for (I i = 0; i < n; i++) { // pass 1: a node all of whose neighbours are free becomes a root
        if (agg[i]) continue;
        bool has_neighbours = false, has_aggregated = false;
        for (I jj = H.row_offsets[i]; jj < H.row_offsets[i + 1]; jj++) {
            const I j = H.column_indices[jj];
            if (j != i) {
                has_neighbours = true;
                if (agg[j]) {
                    has_aggregated = true;
                    break;
                }
            }
        }
        if (!has_neighbours) agg[i] = -n;
        else if (!has_aggregated) {
            agg[i] = next;
            root[next - 1] = i;
            for (I jj = H.row_offsets[i]; jj < H.row_offsets[i + 1]; jj++) agg[H.column_indices[jj]] = next;
            next++;
        }
    }
    for (I i = 0; i < n; i++) { // pass 2: a free node joins a neighbouring aggregate
        if (agg[i]) continue;
        for (I jj = H.row_offsets[i]; jj < H.row_offsets[i + 1]; jj++) {
            const I tj = agg[H.column_indices[jj]];
            if (tj > 0) {
                agg[i] = -tj;
                break;
            }
        }
    }
    next--;
    for (I i = 0; i < n; i++) { // pass 3: renumber from 0; what is still free forms aggregates of its own
        const I ti = agg[i];
        if (ti != 0) {
            agg[i] = ti > 0 ? ti - 1 : (ti == -n ? I(-1) : -ti - 1);
            continue;
        }
        agg[i] = next;
        root[next] = i;
        for (I jj = H.row_offsets[i]; jj < H.row_offsets[i + 1]; jj++)
            if (agg[H.column_indices[jj]] == 0) agg[H.column_indices[jj]] = next;
        next++;
    }
    root.resize(static_cast<size_t>(next));
    aggregates = agg;
    roots = root;
}
template <typename MatrixType, typename ArrayType> void standard_aggregate(const MatrixType &C, ArrayType &aggregates)
{
    cusp::array1d<typename MatrixType::index_type, cusp::host_memory> roots;
    standard_aggregate(C, aggregates, roots);
}
template <typename MatrixType, typename ArrayType> void aggregate(const MatrixType &C, ArrayType &aggregates) { standard_aggregate(C, aggregates); }

namespace detail {

template <typename Csr, typename ArrayType1, typename ArrayType2> void mis_aggregate(const Csr &C, ArrayType1 &aggregates, ArrayType2 &mis, uint64_t seed, cusp::host_memory)
{
    const size_t n = C.num_rows;
    const uint64_t index_mask = 0x7FFFFFFFull;
    std::vector<int> flag, agg(n, -1);
    size_t rounds = 0;
    const size_t total = cusp::graph::detail::mis_host(C, flag, 2, seed, &rounds);
    std::vector<uint64_t> x(n), y, z;
    for (size_t i = 0; i < n; i++) x[i] = (static_cast<uint64_t>(flag[i]) << 31) | static_cast<uint64_t>(i);
    cusp::graph::detail::ring_max(C, x, y);
    for (size_t i = 0; i < n; i++) y[i] += static_cast<uint64_t>(flag[i]) << 31; // the reference's boost
    cusp::graph::detail::ring_max(C, y, z);
    std::vector<int> number(n), members(total, 0), renumbered(total, -1);
    for (size_t i = 0, at = 0; i < n; i++) {
        number[i] = static_cast<int>(at);
        at += flag[i];
    }
    for (size_t i = 0; i < n; i++)
        if ((z[i] >> 31) != 0) { // (a top part of 0: no set node within two steps)
            agg[i] = number[z[i] & index_mask];
            members[agg[i]]++;
        }
    int next = 0;
    for (size_t a = 0; a < total; a++)
        if (members[a] >= 2) renumbered[a] = next++;
    for (size_t i = 0; i < n; i++)
        if (agg[i] >= 0) agg[i] = renumbered[agg[i]];
    aggregates = cusp::array1d<int, cusp::host_memory>(agg);
    mis = cusp::array1d<int, cusp::host_memory>(flag);
}
template <typename Csr, typename ArrayType1, typename ArrayType2> void mis_aggregate(const Csr &C, ArrayType1 &aggregates, ArrayType2 &mis, uint64_t seed, cusp::device_memory)
{
    static_assert(sizeof(typename Csr::index_type) == 4, "the device path takes 32-bit indices");
    cusp::array1d<int, cusp::device_memory> agg(C.num_rows), flag(C.num_rows);
    int64_t count = 0;
    cusp::detail::check(cmi_csr_mis_aggregate((int64_t)C.num_rows, (int64_t)C.num_entries, C.row_offsets.data(), C.column_indices.data(), seed, agg.data(), flag.data(),
                                              &count, nullptr));
    aggregates = agg;
    mis = flag;
}

// the form that takes the seed
template <typename MatrixType, typename ArrayType1, typename ArrayType2> void mis_aggregate(const MatrixType &C, ArrayType1 &aggregates, ArrayType2 &mis, uint64_t seed)
{
    if (C.num_rows != C.num_cols) throw cusp::invalid_input_exception("mis_aggregate: matrix must be square");
    cusp::graph::detail::with_csr(C, [&](const auto &csr) { mis_aggregate(csr, aggregates, mis, seed, typename MatrixType::memory_space()); return 0; },
                                  typename MatrixType::format());
}

} // namespace detail

template <typename MatrixType, typename ArrayType1, typename ArrayType2> void mis_aggregate(const MatrixType &C, ArrayType1 &aggregates, ArrayType2 &mis)
{
    detail::mis_aggregate(C, aggregates, mis, 0);
}
template <typename MatrixType, typename ArrayType> void mis_aggregate(const MatrixType &C, ArrayType &aggregates)
{
    cusp::array1d<int, typename MatrixType::memory_space> mis;
    detail::mis_aggregate(C, aggregates, mis, 0);
}

} // namespace aggregation
} // namespace precond
} // namespace cusp
