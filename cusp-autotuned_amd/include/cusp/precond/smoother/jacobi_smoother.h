// cusp/precond/smoother/jacobi_smoother.h -- jacobi_smoother<ValueType, MemorySpace>: the smoother of a multigrid level
// (reference cusp/precond/smoother/jacobi_smoother.h).  Weight omega = (4/3) / rho(D^-1 A).
//   presmooth(A, b, x)  : x = omega * b / d, the product first -- a Jacobi sweep from x = 0 without its multiply (the reference's
//                         jacobi_presmooth_functor); device_memory: cmi_relax_jacobi_presmooth_*.
//   postsmooth(A, b, x) : one cusp::relaxation::jacobi sweep.
// Every path returns the bits of the host path.  Not built: polynomial, Gauss-Seidel and SOR smoother wrappers.
#pragma once
#include "../../eigen/spectral_radius.h"
#include "../../relaxation/jacobi.h"

namespace cusp {
namespace precond {

template <typename ValueType, typename MemorySpace> class jacobi_smoother {
public:
    cusp::relaxation::jacobi<ValueType, MemorySpace> M;

    jacobi_smoother() {}
    // rho_Dinv_A == 0: estimated here
    template <typename MatrixType> jacobi_smoother(const MatrixType &A, double rho_Dinv_A = 0.0) { initialize(A, rho_Dinv_A); }
    template <typename MemorySpace2> jacobi_smoother(const jacobi_smoother<ValueType, MemorySpace2> &o) : M(o.M) {}

    template <typename MatrixType> void initialize(const MatrixType &A, double rho_Dinv_A = 0.0)
    {
        if (rho_Dinv_A == 0.0) rho_Dinv_A = cusp::eigen::estimate_rho_Dinv_A(A);
        M = cusp::relaxation::jacobi<ValueType, MemorySpace>(A, static_cast<ValueType>((4.0 / 3.0) / rho_Dinv_A));
    }

    template <typename MatrixType, typename VectorType1, typename VectorType2> void presmooth(const MatrixType &, const VectorType1 &b, VectorType2 &x)
    {
        if (b.size() != M.diagonal.size() || x.size() != b.size()) throw cusp::invalid_input_exception("jacobi_smoother::presmooth: b and x must have the matrix's size");
        presmooth_in(b, x, MemorySpace());
    }
    template <typename MatrixType, typename VectorType1, typename VectorType2> void postsmooth(const MatrixType &A, const VectorType1 &b, VectorType2 &x) { M(A, b, x); }

private:
    template <typename VectorType1, typename VectorType2> void presmooth_in(const VectorType1 &b, VectorType2 &x, cusp::host_memory)
    {
        for (size_t i = 0; i < x.size(); i++) {
            const ValueType product = M.default_omega * ValueType(b[i]);
            x[i] = product / M.diagonal[i];
        }
    }
    template <typename VectorType1, typename VectorType2> void presmooth_in(const VectorType1 &b, VectorType2 &x, cusp::device_memory)
    {
        cusp::detail::check(cusp::detail::by_type<ValueType>(cmi_relax_jacobi_presmooth_f64, cmi_relax_jacobi_presmooth_f32)(
            (int64_t)x.size(), M.diagonal.data(), b.data(), M.default_omega, x.data(), nullptr));
    }
};

} // namespace precond
} // namespace cusp
