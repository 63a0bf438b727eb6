// cusp/relaxation/sor.h -- cusp::relaxation::sor<ValueType, MemorySpace>: successive over-relaxation as the reference
// defines it (cusp/relaxation/sor.h, detail/sor.inl): a whole Gauss-Seidel sweep, then a blend with the x from before it,
//   temp = x;  gs(A, b, x, direction);  x = (1 - omega) * temp + omega * x        (cusp::blas::axpby)
// so the relaxation happens after the sweep and later colours read unrelaxed values.  Three calls on both memory spaces; the
// blend is not fused into the sweep's kernel, which would change what later colours read.
#pragma once
#include "gauss_seidel.h"

namespace cusp {
namespace relaxation {

template <typename ValueType, typename MemorySpace> class sor : public cusp::linear_operator<ValueType, MemorySpace> {
    typedef cusp::linear_operator<ValueType, MemorySpace> Parent;

public:
    ValueType default_omega;
    cusp::array1d<ValueType, MemorySpace> temp;
    gauss_seidel<ValueType, MemorySpace> gs;

    sor() : default_omega(0) {}

    template <typename MatrixType>
    sor(const MatrixType &A, const ValueType omega, sweep default_direction = SYMMETRIC)
        : Parent(A.num_rows, A.num_cols, A.num_entries), default_omega(omega), temp(A.num_cols), gs(A, default_direction)
    {
    }

    template <typename MemorySpace2>
    sor(const sor<ValueType, MemorySpace2> &o) : Parent(o.num_rows, o.num_cols, o.num_entries), default_omega(o.default_omega), temp(o.temp), gs(o.gs) {}

    // one step with the constructor's omega and direction
    template <typename MatrixType, typename VectorType1, typename VectorType2> void operator()(const MatrixType &A, const VectorType1 &b, VectorType2 &x)
    {
        (*this)(A, b, x, default_omega, gs.default_direction);
    }

    // one step with the given omega and direction
    template <typename MatrixType, typename VectorType1, typename VectorType2>
    void operator()(const MatrixType &A, const VectorType1 &b, VectorType2 &x, const ValueType omega, sweep direction)
    {
        if (x.size() != A.num_rows) throw cusp::invalid_input_exception("cusp::relaxation::sor: x must have A's size");
        if (temp.size() != x.size()) temp.resize(x.size());
        cusp::blas::copy(x, temp); // temp = x, without the synchronisation a device array's assignment ends with
        gs(A, b, x, direction);
        cusp::blas::axpby(temp, x, x, ValueType(1) - omega, omega);
    }
};

} // namespace relaxation
} // namespace cusp
