// cusp/detail/lu.h -- lu_factor, lu_solve and lu_solver<ValueType, MemorySpace>: the dense coarse-grid solve of a multigrid
// hierarchy (reference cusp/detail/lu.h).  Dense LU with partial pivoting (the first row of largest magnitude), computed and
// applied on the HOST in both memory spaces: the coarse matrix has a few hundred rows at most.
// Deviation from the reference: a zero pivot throws cusp::runtime_exception (the reference returns an error code that its
// caller ignores).
#pragma once
#include <cmath>
#include <vector>

#include "../array1d.h"
#include "../array2d.h"
#include "../convert.h"
#include "../exception.h"

namespace cusp {
namespace detail {

// A (n x n, row-major in a vector) is overwritten by L (unit diagonal, below) and U; pivot[k] = the row exchanged with k
template <typename V> void lu_factor(std::vector<V> &A, std::vector<int> &pivot, size_t n)
{
    pivot.resize(n);
    for (size_t k = 0; k < n; k++) {
        size_t p = k;
        for (size_t i = k + 1; i < n; i++)
            if (std::abs(A[i * n + k]) > std::abs(A[p * n + k])) p = i;
        if (A[p * n + k] == V(0)) throw cusp::runtime_exception("cusp::detail::lu_factor: the matrix is singular");
        pivot[k] = static_cast<int>(p);
        if (p != k)
            for (size_t j = 0; j < n; j++) std::swap(A[k * n + j], A[p * n + j]);
        for (size_t i = k + 1; i < n; i++) {
            const V l = A[i * n + k] / A[k * n + k];
            A[i * n + k] = l;
            for (size_t j = k + 1; j < n; j++) A[i * n + j] = A[i * n + j] - l * A[k * n + j];
        }
    }
}
template <typename V> void lu_solve(const std::vector<V> &LU, const std::vector<int> &pivot, const std::vector<V> &b, std::vector<V> &x, size_t n)
{
    x = b;
    for (size_t k = 0; k < n; k++) std::swap(x[k], x[pivot[k]]);
    for (size_t i = 0; i < n; i++)
        for (size_t j = 0; j < i; j++) x[i] = x[i] - LU[i * n + j] * x[j];
    for (size_t i = n; i-- > 0;) {
        for (size_t j = i + 1; j < n; j++) x[i] = x[i] - LU[i * n + j] * x[j];
        x[i] = x[i] / LU[i * n + i];
    }
}

template <typename ValueType, typename MemorySpace> class lu_solver {
    std::vector<ValueType> lu;
    std::vector<int> pivot;
    size_t n = 0;

public:
    lu_solver() {}
    template <typename MatrixType> lu_solver(const MatrixType &A) { initialize(A); }
    template <typename MemorySpace2> lu_solver(const lu_solver<ValueType, MemorySpace2> &o) : lu(o.factors()), pivot(o.pivots()), n(o.size()) {}
    const std::vector<ValueType> &factors() const { return lu; }
    const std::vector<int> &pivots() const { return pivot; }
    size_t size() const { return n; }

    template <typename MatrixType> void initialize(const MatrixType &A)
    {
        if (A.num_rows != A.num_cols) throw cusp::invalid_input_exception("lu_solver: matrix must be square");
        host_csr<typename MatrixType::index_type, typename MatrixType::value_type> H;
        to_host_csr(A, H, typename MatrixType::format());
        n = A.num_rows;
        lu.assign(n * n, ValueType(0));
        for (size_t i = 0; i < n; i++)
            for (auto q = H.row_offsets[i]; q < H.row_offsets[i + 1]; q++) lu[i * n + H.column_indices[q]] += H.values[q];
        lu_factor(lu, pivot, n);
    }
    // x = A^-1 b; b and x in either space (copied to the host and back)
    template <typename VectorType1, typename VectorType2> void operator()(const VectorType1 &b, VectorType2 &x) const
    {
        if (b.size() != n) throw cusp::invalid_input_exception("lu_solver: b must have the matrix's size");
        const std::vector<ValueType> hb = host_copy(b);
        cusp::array1d<ValueType, cusp::host_memory> hx(n);
        std::vector<ValueType> sol;
        lu_solve(lu, pivot, hb, sol, n);
        for (size_t i = 0; i < n; i++) hx[i] = sol[i];
        x = hx;
    }
};

} // namespace detail
} // namespace cusp
