// cusp/permutation_matrix.h -- cusp::permutation_matrix<IndexType, MemorySpace>: a square permutation held as one index array
// (reference cusp/permutation_matrix.h:107-194).
//   num_rows, num_cols, num_entries (all N) and `permutation` (N indices)
//   permutation_matrix(), (n) the identity, (n, array) a copy of the array, (other memory space's matrix); resize(n): the identity
//   P.symmetric_permute(A)    A <- P A P^T for a square matrix of any of the five formats in P's memory space, through COO as
//                             in the reference: new row = permutation[row], new column = permutation[column], then
//                             sort_by_row_and_column, then the assignment back.  device_memory: two cmi_gather_i32 and the
//                             library's COO sort; a COO copy of A is allocated on the way.
//   cusp::multiply(P, x, y)   y[i] = x[permutation[i]]                        (the reference's gather)
//   cusp::multiply(x, P, y)   y[permutation[i]] = x[i]: the vector that goes with a symmetrically permuted matrix --
//                             (P A P^T) multiply(x, P, .) = multiply(A x, P, .)
// device_memory: cmi_gather_* / cmi_scatter_* (int, float and double values).  An index outside [0, N) throws
// cusp::invalid_input_exception in both spaces; that the array is a bijection is the caller's promise.
// Not here: permutation_matrix_view, products of P with a sparse matrix, convert() from a permutation.
#pragma once
#include <type_traits>

#include "array1d.h"
#include "coo_matrix.h"
#include "exception.h"
#include "format.h"

namespace cusp {

struct permutation_format : known_format {};

namespace detail {

// out[i] = in[map[i]] (scatter: out[map[i]] = in[i]); `out` is sized by the caller and must not be `in`
template <typename Map, typename In, typename Out> void map_copy(bool scatter, const Map &map, const In &in, Out &out, cusp::host_memory)
{
    const size_t m = scatter ? out.size() : in.size();
    for (size_t i = 0; i < map.size(); i++) {
        const auto j = map[i];
        if (j < 0 || static_cast<size_t>(j) >= m) throw cusp::invalid_input_exception("permutation: an index lies outside [0, N)");
        if (scatter) out[j] = in[i];
        else out[i] = in[j];
    }
}
template <typename Map, typename In, typename Out> void map_copy(bool scatter, const Map &map, const In &in, Out &out, cusp::device_memory)
{
    static_assert(sizeof(typename Map::value_type) == 4, "the device path takes 32-bit indices");
    static_assert(std::is_same<typename std::remove_const<typename In::value_type>::type, typename Out::value_type>::value, "the device path moves values of one type");
    const int64_t n = (int64_t)map.size(), m = (int64_t)(scatter ? out.size() : in.size());
    typedef typename Out::value_type T; // int (index arrays), float or double
    using cusp::detail::by_type;
    if constexpr (std::is_same<T, int>::value)
        cusp::detail::check((scatter ? cmi_scatter_i32 : cmi_gather_i32)(n, m, map.data(), in.data(), out.data(), nullptr));
    else
        cusp::detail::check((scatter ? by_type<T>(cmi_scatter_f64, cmi_scatter_f32) : by_type<T>(cmi_gather_f64, cmi_gather_f32))(n, m, map.data(), in.data(), out.data(), nullptr));
}

} // namespace detail

template <typename IndexType, typename MemorySpace> class permutation_matrix : public detail::matrix_base<IndexType, IndexType, MemorySpace, permutation_format> {
    typedef detail::matrix_base<IndexType, IndexType, MemorySpace, permutation_format> Parent;

public:
    typedef cusp::array1d<IndexType, MemorySpace> permutation_array_type;
    typedef permutation_matrix<IndexType, MemorySpace> container;
    template <typename Space> struct rebind { typedef permutation_matrix<IndexType, Space> type; };

    permutation_array_type permutation;

    permutation_matrix() {}
    permutation_matrix(const size_t num_rows) : Parent(num_rows, num_rows, num_rows) { set_identity(num_rows); }
    template <typename MemorySpace2>
    permutation_matrix(const permutation_matrix<IndexType, MemorySpace2> &matrix) : Parent(matrix.num_rows, matrix.num_cols, matrix.num_entries), permutation(matrix.permutation) {}
    template <typename ArrayType> permutation_matrix(const size_t num_rows, const ArrayType &perm) : Parent(num_rows, num_rows, num_rows), permutation(perm)
    {
        if (permutation.size() != num_rows) throw cusp::invalid_input_exception("permutation_matrix: the array must have num_rows elements");
    }

    void resize(const size_t num_rows)
    {
        Parent::resize(num_rows, num_rows, num_rows);
        set_identity(num_rows);
    }
    void swap(permutation_matrix &matrix)
    {
        Parent::swap(matrix);
        permutation.swap(matrix.permutation);
    }

    template <typename MatrixType> void symmetric_permute(MatrixType &matrix) const
    {
        static_assert(std::is_same<typename MatrixType::memory_space, MemorySpace>::value, "symmetric_permute: the matrix lives in the permutation's memory space");
        if (matrix.num_rows != matrix.num_cols || matrix.num_rows != this->num_rows)
            throw cusp::invalid_input_exception("permutation_matrix::symmetric_permute: the matrix must be square and of the permutation's size");
        cusp::coo_matrix<typename MatrixType::index_type, typename MatrixType::value_type, MemorySpace> B(matrix);
        cusp::array1d<typename MatrixType::index_type, MemorySpace> moved(B.num_entries);
        detail::map_copy(false, B.row_indices, permutation, moved, MemorySpace());
        B.row_indices.swap(moved);
        detail::map_copy(false, B.column_indices, permutation, moved, MemorySpace());
        B.column_indices.swap(moved);
        B.sort_by_row_and_column();
        matrix = B;
    }

private:
    void set_identity(size_t n)
    {
        cusp::array1d<IndexType, cusp::host_memory> id(n);
        for (size_t i = 0; i < n; i++) id[i] = (IndexType)i;
        permutation = id;
    }
};

// y[i] = x[permutation[i]]
template <typename IndexType, typename MemorySpace, typename Vector1, typename Vector2>
void multiply(const permutation_matrix<IndexType, MemorySpace> &P, const Vector1 &x, Vector2 &y)
{
    if (x.size() != P.num_rows || y.size() != P.num_rows || P.permutation.size() != P.num_rows)
        throw cusp::invalid_input_exception("cusp::multiply(P, x, y): sizes do not match");
    detail::map_copy(false, P.permutation, x, y, MemorySpace());
}
// y[permutation[i]] = x[i]
template <typename IndexType, typename MemorySpace, typename Vector1, typename Vector2>
void multiply(const Vector1 &x, const permutation_matrix<IndexType, MemorySpace> &P, Vector2 &y)
{
    if (x.size() != P.num_rows || y.size() != P.num_rows || P.permutation.size() != P.num_rows)
        throw cusp::invalid_input_exception("cusp::multiply(x, P, y): sizes do not match");
    detail::map_copy(true, P.permutation, x, y, MemorySpace());
}

} // namespace cusp
