// cusp/precond/aggregation/aggregate.h -- standard_aggregate(C, aggregates[, roots]) and aggregate(C, aggregates)
// (reference cusp/precond/aggregation/aggregate.h; system/detail/sequential/standard_aggregate.h): the three-pass sequential
// aggregation on the structure of the strength matrix C; aggregates[i] = -1 for a node without neighbours.
// Set-up work on the host in BOTH memory spaces, on a host copy of C's structure (the precedent is
// cusp::graph::vertex_coloring); the result is copied into `aggregates`' space.  Known gap: no device aggregation
// (the reference's MIS(2) path), DESIGN 9.
#pragma once
#include "../../array1d.h"
#include "../../convert.h"
#include "../../exception.h"

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

} // namespace aggregation
} // namespace precond
} // namespace cusp
