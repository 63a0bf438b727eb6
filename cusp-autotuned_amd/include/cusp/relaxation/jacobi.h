// cusp/relaxation/jacobi.h -- cusp::relaxation::jacobi<ValueType, MemorySpace>: one weighted Jacobi sweep,
//   x <- x + omega * D^-1 * (b - A x)        (reference cusp/relaxation/jacobi.h, detail/jacobi.inl:77-87)
// evaluated per element as x[i] + omega * (b[i] - y[i]) / d[i] with y = A x: omega * (b - y) first, then the division
// (the reference's jacobi_relax_functor, jacobi.inl:44).
//
//   host_memory   : cusp::multiply(A, x, temp), then that expression in a loop.
//   device_memory : cusp::multiply(A, x, temp) -- the matrix's planned multiply, any of the five formats -- then
//                   cmi_relax_jacobi_update_*, the expression in place in one elementwise launch; x's storage does not move.
// The one-launch form for CSR, cmi_csr_jacobi_sweep_* (the row sum and the expression in the lane that owns the row), is in
// the C-ABI but NOT used here: on the 5-point Poisson matrix it measured 1.16 (f64) and 1.28 (f32) times the two launches
// above once its copy back into x is counted, 1.01 / 1.17 without (profiles/r06_relax_bench.txt).
// Every path returns the bits of the host path (given a multiply whose sums are in storage order: Plan info
// storage_order_sums).  A zero on the diagonal gives what IEEE division gives, as in the reference.
#pragma once
#include "../blas/blas.h"
#include "../format_utils.h"
#include "../linear_operator.h"
#include "../multiply.h"

namespace cusp {
namespace relaxation {

template <typename ValueType, typename MemorySpace> class jacobi : public cusp::linear_operator<ValueType, MemorySpace> {
    typedef cusp::linear_operator<ValueType, MemorySpace> Parent;

public:
    ValueType default_omega;
    cusp::array1d<ValueType, MemorySpace> diagonal;
    cusp::array1d<ValueType, MemorySpace> temp;

    jacobi() : default_omega(0) {}

    template <typename MatrixType>
    jacobi(const MatrixType &A, ValueType omega = ValueType(1)) : Parent(A.num_rows, A.num_cols, A.num_rows), default_omega(omega), temp(A.num_rows)
    {
        cusp::extract_diagonal(A, diagonal); // set-up work: read from a host copy of the matrix
    }

    template <typename MemorySpace2>
    jacobi(const jacobi<ValueType, MemorySpace2> &o) : Parent(o.num_rows, o.num_cols, o.num_entries), default_omega(o.default_omega), diagonal(o.diagonal), temp(o.temp) {}

    // one sweep with the constructor's omega
    template <typename MatrixType, typename VectorType1, typename VectorType2> void operator()(const MatrixType &A, const VectorType1 &b, VectorType2 &x)
    {
        (*this)(A, b, x, default_omega);
    }

    // one sweep with the given omega
    template <typename MatrixType, typename VectorType1, typename VectorType2>
    void operator()(const MatrixType &A, const VectorType1 &b, VectorType2 &x, const ValueType omega)
    {
        if (A.num_rows != A.num_cols || b.size() != A.num_rows || x.size() != A.num_rows || diagonal.size() != A.num_rows)
            throw cusp::invalid_input_exception("cusp::relaxation::jacobi: A must be the square matrix this object was made from, b and x of its size");
        if (temp.size() != A.num_rows) temp.resize(A.num_rows);
        sweep(A, b, x, omega, MemorySpace());
    }

private:
    template <typename MatrixType, typename VectorType1, typename VectorType2>
    void sweep(const MatrixType &A, const VectorType1 &b, VectorType2 &x, ValueType omega, cusp::host_memory)
    {
        cusp::multiply(A, x, temp);
        for (size_t i = 0; i < x.size(); i++) {
            const ValueType xi = x[i], bi = b[i], yi = temp[i], di = diagonal[i];
            x[i] = xi + omega * (bi - yi) / di;
        }
    }
    template <typename MatrixType, typename VectorType1, typename VectorType2>
    void sweep(const MatrixType &A, const VectorType1 &b, VectorType2 &x, ValueType omega, cusp::device_memory)
    {
        static_assert(std::is_same<ValueType, double>::value || std::is_same<ValueType, float>::value,
                      "device_memory cusp::relaxation::jacobi is implemented for float and double");
        if (A.num_rows == 0) return;
        cusp::multiply(A, x, temp);
        cusp::detail::check(cusp::detail::by_type<ValueType>(cmi_relax_jacobi_update_f64, cmi_relax_jacobi_update_f32)(
            (int64_t)x.size(), diagonal.data(), b.data(), temp.data(), omega, x.data(), nullptr));
    }
};

} // namespace relaxation
} // namespace cusp
