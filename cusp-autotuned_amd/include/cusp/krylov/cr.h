// cusp/krylov/cr.h -- cusp::krylov::cr(A, x, b[, monitor[, M]]): the conjugate residual method for symmetric (possibly indefinite) systems
// (reference cusp/krylov/cr.h, detail/cr.inl:38-125 -- the same operation order: alpha = <r, A z> / <A p, A p>, the residual recomputed from
// b - A x every 8th iteration, y = A p updated by recurrence).  A caller of the hot path: one or two cusp::multiply(A, ., .) per iteration.
#pragma once
#include <cmath>
#include <cstdlib>

#include "../array1d.h"
#include "../blas/blas.h"
#include "../linear_operator.h"
#include "../monitor.h"
#include "../multiply.h"
#include "cg.h"

namespace cusp {
namespace krylov {
namespace detail {

// ---- device_memory, identity preconditioner: the fused iteration (csrc/blas1_extra.hip cmi_cr_*) ----------------------------------------

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor>
void cr_fused_device(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor)
{
    typedef typename LinearOperator::value_type T;
    typedef cusp::array1d<T, cusp::device_memory> Vec;
    const size_t N = A.num_rows, recompute_r = 8;
    Vec y(N), r(N), p(N), Az(N), Ax(N);
    cusp::array1d<double, cusp::device_memory> scalars(4); // <r, A r>[0], [1], <A p, A p>, <r, r>
    double *rz[2] = {scalars.data(), scalars.data() + 1};
    double *yy = scalars.data() + 2, *rr = scalars.data() + 3;
    cusp::blas::detail::device_workspace &w = cusp::blas::detail::workspace();
    pinned_scalar rr_host;
    cusp::multiply(A, x, Ax);
    cusp::blas::axpby(b, Ax, r, T(1), T(-1));
    cusp::blas::copy(r, p);
    multiply_dot(A, r, Az, r, rz[0], w.ws); // A r and <A r, r>
    cusp::blas::copy(Az, y);                                            // y = A p (p == r at the start)
    cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, y.data(), y.data(), yy, w.ws, nullptr));
    cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, r.data(), r.data(), rr, w.ws, nullptr));
    rr_host.fetch(rr);
    int cur = 0;
    while (!monitor.finished_norm(static_cast<typename Monitor::Real>(std::sqrt(rr_host.wait())))) { // the one host read; the previous iteration's multiply
        const size_t iter = monitor.iteration_count();                                                   // and py-pass are still running behind it
        const bool update_r = (iter % recompute_r) && iter > 0;
        cusp::detail::check(by_type<T>(cmi_cr_xr_f64, cmi_cr_xr_f32)(N, rz[cur], yy, p.data(), y.data(), x.data(), r.data(), update_r ? 1 : 0, rr, rr_host.host, w.ws, nullptr));
        if (update_r) rr_host.record();
        else { // every 8th iteration the residual is rebuilt from b - A x (cr.inl:96-107)
            cusp::multiply(A, x, Ax);
            cusp::blas::axpby(b, Ax, r, T(1), T(-1));
            cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, r.data(), r.data(), rr, w.ws, nullptr));
            rr_host.fetch(rr);
        }
        multiply_dot(A, r, Az, r, rz[cur ^ 1], w.ws); // the hot path: A r and <A r, r>
        cusp::detail::check(by_type<T>(cmi_cr_py_f64, cmi_cr_py_f32)(N, rz[cur ^ 1], rz[cur], r.data(), Az.data(), p.data(), y.data(), yy, w.ws, nullptr));
        cur ^= 1;
        ++monitor;
    }
    cusp::detail::check(cmi_device_synchronize());
}

} // namespace detail

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename Preconditioner,
          typename = detail::not_policy<LinearOperator>>
void cr(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor, Preconditioner &M)
{
    typedef typename LinearOperator::value_type ValueType;
    typedef typename LinearOperator::memory_space MemorySpace;
    if (A.num_rows != A.num_cols) throw cusp::invalid_input_exception("cr: the operator must be square");
    if constexpr (detail::fused_eligible<LinearOperator, VectorType1, Monitor>::value && detail::is_identity<Preconditioner>::value &&
                  cusp::detail::has_format<LinearOperator>::value) {
        const char *e = std::getenv("CMI_CR_FUSED");
        if (!(e && e[0] == '0')) { detail::cr_fused_device(A, x, b, monitor); return; } // ('0': measurements, the operation-by-operation path below)
    }
    const size_t N = A.num_rows, recompute_r = 8; // (cr.inl:50: how often the residual is rebuilt from b - A x)
    const bool plain = detail::is_identity<Preconditioner>::value; // M = identity_operator: z IS r (no copy per iteration)
    cusp::array1d<ValueType, MemorySpace> y(N), z_own(plain ? 0 : N), r(N), p(N), Az(N), Ax(N);
    cusp::array1d<ValueType, MemorySpace> &z = plain ? r : z_own;

    cusp::multiply(A, x, Ax);
    cusp::blas::axpby(b, Ax, r, ValueType(1), ValueType(-1)); // r <- b - A x
    if (!plain) detail::apply(M, r, z, 0);                    // z <- M r
    cusp::blas::copy(z, p);
    cusp::multiply(A, p, y);                                  // y <- A p
    cusp::multiply(A, z, Az);
    ValueType rz = cusp::blas::dotc(r, Az);                   // <r, A z>

    while (!monitor.finished(r)) {
        const ValueType alpha = rz / cusp::blas::dotc(y, y);
        cusp::blas::axpy(p, x, alpha);                        // x <- x + alpha p
        const size_t iter = monitor.iteration_count();
        if ((iter % recompute_r) && iter > 0) {
            cusp::blas::axpy(y, r, -alpha);                   // r <- r - alpha A p
        } else {
            cusp::multiply(A, x, Ax);
            cusp::blas::axpby(b, Ax, r, ValueType(1), ValueType(-1));
        }
        if (!plain) detail::apply(M, r, z, 0);
        cusp::multiply(A, z, Az);
        const ValueType rz_old = rz;
        rz = cusp::blas::dotc(r, Az);
        const ValueType beta = rz / rz_old;
        cusp::blas::axpby(z, p, p, ValueType(1), beta);       // p <- z + beta p
        cusp::blas::axpby(Az, y, y, ValueType(1), beta);      // y = A p <- A z + beta y
        ++monitor;
    }
}

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename = detail::not_policy<LinearOperator>>
void cr(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor)
{
    cusp::identity_operator<typename LinearOperator::value_type, typename LinearOperator::memory_space> M(A.num_rows, A.num_cols);
    cusp::krylov::cr(A, x, b, monitor, M);
}
template <typename LinearOperator, typename VectorType1, typename VectorType2, typename = detail::not_policy<LinearOperator>>
void cr(const LinearOperator &A, VectorType1 &x, const VectorType2 &b)
{
    cusp::monitor<typename LinearOperator::value_type> monitor(b);
    cusp::krylov::cr(A, x, b, monitor);
}
template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename Preconditioner>
void cr(const cusp::execution_policy<Derived> &, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor, Preconditioner &M)
{ cusp::krylov::cr(A, x, b, monitor, M); }
template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor>
void cr(const cusp::execution_policy<Derived> &, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor)
{ cusp::krylov::cr(A, x, b, monitor); }

} // namespace krylov
} // namespace cusp
