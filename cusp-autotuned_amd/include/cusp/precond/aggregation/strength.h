// cusp/precond/aggregation/strength.h -- symmetric_strength_of_connection(A, S, theta = 0) and strength_of_connection
// (reference cusp/precond/aggregation/strength.h; sequential loop system/detail/sequential/symmetric_strength.h).
// S keeps the entries of the square CSR matrix A with |A_ij| >= theta * sqrt(|A_ii| * |A_jj|), in storage order: product and
// square root in the value type, the product with theta and the comparison in double; A_ii is cusp::extract_diagonal's.
//   host_memory   : the reference's sequential loop.
//   device_memory : cmi_csr_strength_symmetric_*; it returns the bits of the host path.
// Not built: evolution strength.
#pragma once
#include <cmath>
#include <vector>

#include "../../csr_matrix.h"
#include "../../format_utils.h"

namespace cusp {
namespace precond {
namespace aggregation {
namespace detail {

template <typename A, typename S> void strength(const A &a, S &s, double theta, cusp::host_memory)
{
    typedef typename S::index_type I;
    typedef typename S::value_type V;
    cusp::array1d<V, cusp::host_memory> d;
    cusp::extract_diagonal(a, d);
    std::vector<I> Sp(a.num_rows + 1, I(0)), Sj;
    std::vector<V> Sx;
    for (size_t i = 0; i < a.num_rows; i++) {
        const V aii = d[i];
        for (auto jj = a.row_offsets[i]; jj < a.row_offsets[i + 1]; jj++) {
            const I j = a.column_indices[jj];
            const V aij = a.values[jj], ajj = (j >= 0 && static_cast<size_t>(j) < a.num_rows) ? d[j] : V(0);
            const V prod = std::abs(aii) * std::abs(ajj);
            const V root = std::sqrt(prod);
            if (static_cast<double>(std::abs(aij)) >= theta * static_cast<double>(root)) {
                Sj.push_back(j);
                Sx.push_back(aij);
            }
        }
        Sp[i + 1] = static_cast<I>(Sj.size());
    }
    s.resize(a.num_rows, a.num_cols, Sj.size());
    for (size_t i = 0; i <= s.num_rows; i++) s.row_offsets[i] = Sp[i];
    for (size_t q = 0; q < Sj.size(); q++) {
        s.column_indices[q] = Sj[q];
        s.values[q] = Sx[q];
    }
}

template <typename A, typename S> void strength(const A &a, S &s, double theta, cusp::device_memory)
{
    typedef typename S::value_type V;
    cusp::csr_matrix<int, V, cusp::device_memory> t(a.num_rows, a.num_cols, a.num_entries);
    const int64_t n = (int64_t)a.num_rows, nnz = (int64_t)a.num_entries; // square: n rows and n columns; t holds up to nnz entries
    cusp::detail::check(cusp::detail::by_type<V>(cmi_csr_strength_symmetric_f64, cmi_csr_strength_symmetric_f32)(
        n, n, nnz, a.row_offsets.data(), a.column_indices.data(), a.values.data(), theta,
                                                                                                                 t.row_offsets.data(), t.column_indices.data(), t.values.data(), nnz, nullptr));
    cusp::detail::take_compacted(t, s);
}

} // namespace detail

template <typename MatrixType1, typename MatrixType2> void symmetric_strength_of_connection(const MatrixType1 &A, MatrixType2 &S, const double theta = 0.0)
{
    static_assert(std::is_same<typename MatrixType1::format, cusp::csr_format>::value && std::is_same<typename MatrixType2::format, cusp::csr_format>::value,
                  "symmetric_strength_of_connection is implemented for csr matrices: cusp::convert first");
    static_assert(std::is_same<typename MatrixType1::memory_space, typename MatrixType2::memory_space>::value, "symmetric_strength_of_connection: A and S must live in one memory space");
    if (A.num_rows != A.num_cols) throw cusp::invalid_input_exception("symmetric_strength_of_connection: matrix must be square");
    detail::strength(A, S, theta, typename MatrixType2::memory_space());
}
template <typename MatrixType1, typename MatrixType2> void strength_of_connection(const MatrixType1 &A, MatrixType2 &S, const double theta = 0.0)
{
    symmetric_strength_of_connection(A, S, theta);
}

} // namespace aggregation
} // namespace precond
} // namespace cusp
