// cusp/krylov/bicgstab.h -- cusp::krylov::bicgstab(A, x, b[, monitor[, M]]): the stabilised bi-conjugate gradient method for
// non-symmetric systems, right-preconditioned (reference cusp/krylov/bicgstab.h, detail/bicgstab.inl:48-128 -- the same operation order, so the
// same iteration counts: alpha from <r*, A M p>, the early exit on s, omega from <A M s, s> / <A M s, A M s>, x and p updated with axpbypcz).
// Another CALLER of the hot path: two cusp::multiply(A, ., .) per iteration through A's plan, everything else cusp::blas (device_memory: the
// library's kernels; the scalars make four 8-byte reads per iteration, as the reference's Thrust reductions do).  Any memory space, any format,
// any M with operator()(x, y) or a matrix.
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

// ---- device_memory, identity preconditioner: the fused iteration (csrc/blas1_extra.hip cmi_bicgstab_*) --------------------------------
// y <- A v and *out <- <y, w> for any w: CSR in ONE launch through the container's plan (cmi_spmv_csr_dot_plan_*), the other formats multiply + dot
template <typename A, typename V> void multiply_dot_w(const A &a, const V &v, V &y, const V &w, double *out, void *ws, cusp::csr_format)
{
    cusp::detail::require_int_index<A>();
    if (const cmi_plan *pl = cusp::detail::plan_of(a, nullptr, 0))
        cusp::detail::check(by_type<typename A::value_type>(cmi_spmv_csr_dot_plan_f64, cmi_spmv_csr_dot_plan_f32)(
            pl, a.row_offsets.data(), a.column_indices.data(), a.values.data(),
                                                                                                                  v.data(), y.data(), w.data(), out, ws, nullptr));
    else
        multiply_then_dot(a, v, y, w, out, ws);
}
template <typename A, typename V, typename Format> void multiply_dot_w(const A &a, const V &v, V &y, const V &w, double *out, void *ws, Format) { multiply_then_dot(a, v, y, w, out, ws); }

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor>
void bicgstab_fused_device(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor)
{
    typedef typename LinearOperator::value_type T;
    typedef cusp::array1d<T, cusp::device_memory> Vec;
    const size_t N = A.num_rows;
    Vec p(N), r(N), r_star(N), s(N), AMp(N), AMs(N);
    cusp::array1d<double, cusp::device_memory> scalars(7); // rho[0], rho[1], d1 = <r*, A p>, d2 = <A s, s>, d3 = <A s, A s>, <s, s>, <r, r>
    double *rho[2] = {scalars.data(), scalars.data() + 1};
    double *d1 = scalars.data() + 2, *d2 = scalars.data() + 3, *d3 = scalars.data() + 4, *ss = scalars.data() + 5, *rr = scalars.data() + 6;
    cusp::blas::detail::device_workspace &w = cusp::blas::detail::workspace();
    pinned_scalar ss_host, rr_host;
    cusp::multiply(A, x, r);
    cusp::blas::axpby(b, r, r, T(1), T(-1));
    cusp::blas::copy(r, p);
    cusp::blas::copy(r, r_star);
    cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, r_star.data(), r.data(), rho[0], w.ws, nullptr));
    cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, r.data(), r.data(), rr, w.ws, nullptr));
    rr_host.fetch(rr);
    int cur = 0;
    for (;;) {
        multiply_dot_w(A, p, AMp, r_star, d1, w.ws, typename LinearOperator::format());                    // speculative: A p and <r*, A p>
        if (monitor.finished_norm(static_cast<typename Monitor::Real>(std::sqrt(rr_host.wait())))) break;  // ||r||
        cusp::detail::check(by_type<T>(cmi_bicgstab_s_f64, cmi_bicgstab_s_f32)(N, rho[cur], d1, r.data(), AMp.data(), s.data(), ss, ss_host.host, w.ws, nullptr));
        ss_host.record();
        multiply_dot_w(A, s, AMs, s, d2, w.ws, typename LinearOperator::format());                         // speculative: A s and <A s, s>
        if (monitor.finished_norm(static_cast<typename Monitor::Real>(std::sqrt(ss_host.wait())))) {       // ||s||: half a step is enough
            cusp::detail::check(by_type<T>(cmi_blas_axpy_ratio_f64, cmi_blas_axpy_ratio_f32)(N, rho[cur], d1, p.data(), x.data(), nullptr));
            break;
        }
        cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, AMs.data(), AMs.data(), d3, w.ws, nullptr));
        cusp::detail::check(by_type<T>(cmi_bicgstab_xr_f64, cmi_bicgstab_xr_f32)(N, rho[cur], d1, d2, d3, p.data(), s.data(), AMs.data(), r_star.data(), x.data(),
                                                                                 r.data(), rho[cur ^ 1], rr, rr_host.host, w.ws, nullptr));
        rr_host.record();
        cusp::detail::check(by_type<T>(cmi_bicgstab_p_f64, cmi_bicgstab_p_f32)(N, rho[cur ^ 1], rho[cur], d1, d2, d3, r.data(), AMp.data(), p.data(), nullptr));
        cur ^= 1;
        ++monitor;
    }
    cusp::detail::check(cmi_device_synchronize()); // the discarded multiply must not outlive its vectors
}

} // namespace detail

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename Preconditioner,
          typename = detail::not_policy<LinearOperator>>
void bicgstab(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor, Preconditioner &M)
{
    typedef typename LinearOperator::value_type ValueType;
    typedef typename LinearOperator::memory_space MemorySpace;
    if (A.num_rows != A.num_cols) throw cusp::invalid_input_exception("bicgstab: the operator must be square");
    if constexpr (detail::fused_eligible<LinearOperator, VectorType1, Monitor>::value && detail::is_identity<Preconditioner>::value &&
                  cusp::detail::has_format<LinearOperator>::value) {
        const char *e = std::getenv("CMI_BICGSTAB_FUSED");
        if (!(e && e[0] == '0')) { detail::bicgstab_fused_device(A, x, b, monitor); return; } // ('0': measurements, the operation-by-operation path below)
    }
    const size_t N = A.num_rows;
    // M = identity_operator (the default): M p IS p and M s IS s -- the two copies per iteration the reference makes are skipped (aliases below)
    const bool plain = detail::is_identity<Preconditioner>::value;
    cusp::array1d<ValueType, MemorySpace> p(N), r(N), r_star(N), s(N), Mp_own(plain ? 0 : N), AMp(N), Ms_own(plain ? 0 : N), AMs(N);
    cusp::array1d<ValueType, MemorySpace> &Mp = plain ? p : Mp_own, &Ms = plain ? s : Ms_own;

    cusp::multiply(A, x, r);
    cusp::blas::axpby(b, r, r, ValueType(1), ValueType(-1)); // r <- b - A x
    cusp::blas::copy(r, p);
    cusp::blas::copy(r, r_star);                             // the shadow residual stays r_0
    ValueType rho = cusp::blas::dotc(r_star, r);

    while (!monitor.finished(r)) {
        if (!plain) detail::apply(M, p, Mp, 0);
        cusp::multiply(A, Mp, AMp);
        const ValueType alpha = rho / cusp::blas::dotc(r_star, AMp);
        cusp::blas::axpby(r, AMp, s, ValueType(1), -alpha);  // s <- r - alpha A M p
        if (monitor.finished(s)) {                           // half a step is enough
            cusp::blas::axpby(x, Mp, x, ValueType(1), alpha);
            break;
        }
        if (!plain) detail::apply(M, s, Ms, 0);
        cusp::multiply(A, Ms, AMs);
        const ValueType omega = cusp::blas::dotc(AMs, s) / cusp::blas::dotc(AMs, AMs);
        cusp::blas::axpbypcz(x, Mp, Ms, x, ValueType(1), alpha, omega);     // x <- x + alpha M p + omega M s
        cusp::blas::axpby(s, AMs, r, ValueType(1), -omega);                  // r <- s - omega A M s
        const ValueType rho_new = cusp::blas::dotc(r_star, r);
        const ValueType beta = (rho_new / rho) * (alpha / omega);
        rho = rho_new;
        cusp::blas::axpbypcz(r, p, AMp, p, ValueType(1), beta, -beta * omega); // p <- r + beta (p - omega A M p)
        ++monitor;
    }
}

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename = detail::not_policy<LinearOperator>>
void bicgstab(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor)
{
    cusp::identity_operator<typename LinearOperator::value_type, typename LinearOperator::memory_space> M(A.num_rows, A.num_cols);
    cusp::krylov::bicgstab(A, x, b, monitor, M);
}
template <typename LinearOperator, typename VectorType1, typename VectorType2, typename = detail::not_policy<LinearOperator>>
void bicgstab(const LinearOperator &A, VectorType1 &x, const VectorType2 &b)
{
    cusp::monitor<typename LinearOperator::value_type> monitor(b);
    cusp::krylov::bicgstab(A, x, b, monitor);
}
// (the reference's policy-taking forms: the policy selects nothing here -- the containers' memory space does)
template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename Preconditioner>
void bicgstab(const cusp::execution_policy<Derived> &, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor, Preconditioner &M)
{ cusp::krylov::bicgstab(A, x, b, monitor, M); }
template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor>
void bicgstab(const cusp::execution_policy<Derived> &, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor)
{ cusp::krylov::bicgstab(A, x, b, monitor); }

} // namespace krylov
} // namespace cusp
