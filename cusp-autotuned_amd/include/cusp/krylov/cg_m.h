// cusp/krylov/cg_m.h -- cusp::krylov::cg_m(A, x, b, sigma[, monitor]): multi-shift conjugate gradients.  Solves (A + sigma_s I) x_s = b for
// every shift in `sigma` with ONE cusp::multiply per iteration (B. Jegerlehner, hep-lat/9612014; reference cusp/krylov/cg_m.h,
// detail/cg_m.inl -- the same operations in the same order).  x holds N * N_s values, shift s at [s N, (s + 1) N); it is zero-filled on entry.
// The monitor watches the residual of the UNSHIFTED system (sigma = 0), as the reference's does; no shift is stopped or frozen on its own.
//
// Two paths:
//   generic  any memory space, any format or linear operator: operation by operation in ValueType; the per-shift coefficients (zeta, beta,
//            alpha: N_s values each) are formed on the host and, on device_memory, uploaded for cmi_cg_m_update_xp_* (three host reads per
//            iteration, as the reference's dotc calls make).
//   fused    device_memory, float or double, a monitor with finished_norm: cg_fused_device's schedule -- speculative multiply + <y,p>,
//            cmi_cg_update_* (r, <r,r> and its host mirror), cmi_cg_m_coefficients_*, cmi_cg_m_update_xp_*: four launches and ONE host read
//            per iteration, the scalars doubles in device memory.  $CMI_CG_M_FUSED=0 selects the generic path (measurements).
#pragma once
#include <cmath>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include "../array1d.h"
#include "../blas/blas.h"
#include "../execution_policy.h"
#include "../monitor.h"
#include "../multiply.h"
#include "cg.h"

namespace cusp {
namespace krylov {
namespace detail {
namespace multishift {

// KERNEL_ZB of the reference (cg_m.inl:69-97, bicgstab_m.inl:163-189), term for term: the next zeta and this step's beta of one shift,
// with the clamp of a vanishing zeta behind the beta
template <typename T> inline void zb(T beta_m1, T beta_0, T alpha_0, T z0, T zm1, T sigma, T &z1, T &b0)
{
    z1 = z0 * zm1 * beta_m1 / (beta_0 * alpha_0 * (zm1 - z0) + beta_m1 * zm1 * (T(1) - beta_0 * sigma));
    b0 = beta_0 * z1 / z0;
    if (std::abs(z1) < T(1e-30)) z1 = T(1e-18);
}
// KERNEL_A: the shifted alpha
template <typename T> inline T a(T beta_0, T alpha_0, T z0, T z1, T b0) { return alpha_0 / beta_0 * z1 * b0 / z0; }

// dest[s N, (s + 1) N) <- b for every shift (the reference's vectorize_copy)
template <typename T> void replicate(const T *b, T *dest, size_t N, size_t N_s, cusp::host_memory)
{
    for (size_t s = 0; s < N_s; s++)
        for (size_t i = 0; i < N; i++) dest[s * N + i] = b[i];
}
template <typename T> void replicate(const T *b, T *dest, size_t N, size_t N_s, cusp::device_memory)
{
    for (size_t s = 0; s < N_s; s++) cusp::detail::check(by_type<T>(cmi_blas_copy_f64, cmi_blas_copy_f32)(N, b, dest + s * N, nullptr));
}

// KERNEL_XP: x_s <- x_s - beta_s p_s (the old p_s), p_s <- zeta_s r + alpha_s p_s
template <typename T>
void xp(const std::vector<T> &alpha_s, const std::vector<T> &z_1, const std::vector<T> &beta_s, const T *r, T *x, T *ps, size_t N, cusp::host_memory)
{
    for (size_t s = 0; s < alpha_s.size(); s++)
        for (size_t i = 0; i < N; i++) {
            const T p = ps[s * N + i];
            x[s * N + i] = x[s * N + i] - beta_s[s] * p;
            ps[s * N + i] = z_1[s] * r[i] + alpha_s[s] * p;
        }
}
template <typename T>
void xp(const std::vector<T> &alpha_s, const std::vector<T> &z_1, const std::vector<T> &beta_s, const T *r, T *x, T *ps, size_t N, cusp::device_memory)
{
    static_assert(cusp::detail::is_real<T>::value, "device_memory cg_m is implemented for float and double");
    if (alpha_s.empty()) return;
    const cusp::array1d<T, cusp::device_memory> a(alpha_s), z(z_1), b(beta_s); // N_s values each
    cusp::detail::check(by_type<T>(cmi_cg_m_update_xp_f64, cmi_cg_m_update_xp_f32)(N, alpha_s.size(), N, nullptr, b.data(), a.data(), z.data(), r, nullptr, x, ps,
                                                                                   nullptr)); // (no state, no p_0: the shifted part only)
}

template <typename A, typename X, typename B, typename S> void check_sizes(const A &a, const X &x, const B &b, const S &sigma, const char *who)
{
    if (a.num_rows != a.num_cols) throw cusp::invalid_input_exception(std::string(who) + ": matrix must be square");
    if (b.size() != a.num_rows) throw cusp::invalid_input_exception(std::string(who) + ": b does not match the matrix");
    if (x.size() != a.num_rows * sigma.size()) throw cusp::invalid_input_exception(std::string(who) + ": x must hold num_rows values per shift");
}

} // namespace multishift

// reference cusp/krylov/detail/cg_m.inl:386-503, operation by operation (any memory space)
template <typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3, typename Monitor>
void cg_m_plain(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma, Monitor &monitor)
{
    typedef typename LinearOperator::value_type ValueType;
    typedef typename LinearOperator::memory_space MemorySpace;
    const size_t N = A.num_rows, N_s = sigma.size();

    cusp::array1d<ValueType, MemorySpace> p_0_s(N * N_s), r_0(N), p_0(N), Ap(N);
    // the per-shift parameters: N_s values each, kept on the host
    const cusp::array1d<ValueType, cusp::host_memory> sig(sigma);
    std::vector<ValueType> z_m1_s(N_s, ValueType(1)), z_0_s(N_s, ValueType(1)), z_1_s(N_s), alpha_0_s(N_s, ValueType(0)), beta_0_s(N_s);
    ValueType beta_m1, beta_0(1), alpha_0(0), rsq_0, rsq_1;

    cusp::blas::copy(b, r_0);
    rsq_1 = cusp::blas::dotc(r_0, r_0);
    cusp::blas::fill(x, ValueType(0));
    multishift::replicate(b.data(), p_0_s.data(), N, N_s, MemorySpace());
    cusp::blas::copy(b, p_0);

    while (!monitor.finished(r_0)) {
        rsq_0 = rsq_1;
        beta_m1 = beta_0;
        cusp::multiply(A, p_0, Ap);                                    // the one multiply
        const ValueType pAp = cusp::blas::dotc(p_0, Ap);
        beta_0 = -rsq_0 / pAp;
        cusp::blas::axpy(Ap, r_0, beta_0);                             // r <- r + beta_0 A p
        for (size_t s = 0; s < N_s; s++) multishift::zb(beta_m1, beta_0, alpha_0, z_0_s[s], z_m1_s[s], sig[s], z_1_s[s], beta_0_s[s]);
        rsq_1 = cusp::blas::dotc(r_0, r_0);
        alpha_0 = rsq_1 / rsq_0;
        cusp::blas::axpby(r_0, p_0, p_0, ValueType(1), alpha_0);       // p <- r + alpha_0 p
        for (size_t s = 0; s < N_s; s++) alpha_0_s[s] = multishift::a(beta_0, alpha_0, z_0_s[s], z_1_s[s], beta_0_s[s]);
        multishift::xp(alpha_0_s, z_1_s, beta_0_s, r_0.data(), x.data(), p_0_s.data(), N, MemorySpace());
        z_m1_s = z_0_s;                                                // zeta_-1 <- zeta_0, then zeta_0 <- zeta_1
        z_0_s = z_1_s;
        ++monitor;
    }
}

// device_memory: cg_fused_device's schedule with the shifted updates behind the residual update (see the head of this file)
template <typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3, typename Monitor>
void cg_m_fused_device(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma, Monitor &monitor)
{
    typedef typename LinearOperator::value_type T;
    typedef cusp::array1d<T, cusp::device_memory> Vec;
    const size_t N = A.num_rows, N_s = sigma.size();
    Vec y(N), r(N), p0(N), ps(N * N_s);
    const Vec sig(sigma);
    Vec zm1(N_s, T(1)), z0(N_s, T(1)), beta_s(N_s), alpha_s(N_s);
    Vec state(std::vector<T>{T(1), T(0)});                 // (beta_0, alpha_0) of the previous iteration
    cusp::array1d<double, cusp::device_memory> scalars(3); // rr[0], rr[1], <y,p>
    cusp::blas::detail::device_workspace &w = cusp::blas::detail::workspace();
    double *rr[2] = {scalars.data(), scalars.data() + 1};
    double *yp = scalars.data() + 2;
    pinned_scalar rr_host;
    cusp::blas::copy(b, r);
    cusp::blas::copy(b, p0);
    multishift::replicate(b.data(), ps.data(), N, N_s, cusp::device_memory());
    cusp::blas::fill(x, T(0));
    cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, r.data(), r.data(), rr[0], w.ws, nullptr));
    rr_host.fetch(rr[0]);
    int cur = 0;
    for (;;) {
        multiply_dot(A, p0, y, p0, yp, w.ws); // the multiply, speculative: y <- A p0, *yp <- <y, p0>
        if (monitor.finished_norm(static_cast<typename Monitor::Real>(std::sqrt(rr_host.wait())))) break; // the one host read
        cusp::detail::check(by_type<T>(cmi_cg_update_f64, cmi_cg_update_f32)(N, rr[cur], yp, nullptr, y.data(), nullptr, r.data(), rr[cur ^ 1], rr_host.host, w.ws,
                                                                             nullptr)); // r <- r + beta_0 y, <r,r>
        rr_host.record();
        cusp::detail::check(by_type<T>(cmi_cg_m_coefficients_f64, cmi_cg_m_coefficients_f32)(N_s, rr[cur], yp, rr[cur ^ 1], state.data(), sig.data(), zm1.data(),
                                                                                             z0.data(), beta_s.data(), alpha_s.data(), nullptr));
        cusp::detail::check(by_type<T>(cmi_cg_m_update_xp_f64, cmi_cg_m_update_xp_f32)(N, N_s, N, state.data(), beta_s.data(), alpha_s.data(), z0.data(), r.data(),
                                                                                       p0.data(), x.data(), ps.data(),
                                                                                       nullptr)); // (the shifts lie N apart)
        cur ^= 1;
        ++monitor;
    }
    cusp::detail::check(cmi_device_synchronize()); // the discarded multiply must not outlive y
}

} // namespace detail

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3, typename Monitor,
          typename = detail::not_policy<LinearOperator>>
void cg_m(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma, Monitor &monitor)
{
    detail::multishift::check_sizes(A, x, b, sigma, "cg_m");
    if constexpr (detail::fused_eligible<LinearOperator, VectorType1, Monitor>::value &&
                  std::is_same<typename VectorType2::value_type, typename LinearOperator::value_type>::value) {
        const char *e = std::getenv("CMI_CG_M_FUSED");
        if (e && e[0] == '0') detail::cg_m_plain(A, x, b, sigma, monitor); // (measurements: the operation-by-operation path)
        else detail::cg_m_fused_device(A, x, b, sigma, monitor);
    } else {
        detail::cg_m_plain(A, x, b, sigma, monitor);
    }
}

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3, typename = detail::not_policy<LinearOperator>>
void cg_m(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma)
{
    cusp::monitor<typename LinearOperator::value_type> monitor(b);
    cusp::krylov::cg_m(A, x, b, sigma, monitor);
}

// ---- execution-policy overloads (reference cusp/krylov/cg_m.h: cg_m(exec, A, x, b, sigma[, monitor])): a policy derived from
// cusp::execution_policy<Derived> reaches a user `cg_m(my_policy&, ...)` overload by ADL (testing/multi_mass.cu:9-40); a policy without one
// gets the memory-space dispatch above.
namespace detail {
namespace policy_default {
template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3, typename Monitor,
          typename = typename std::enable_if<std::is_base_of<cusp::execution_policy<Derived>, Derived>::value>::type>
void cg_m(Derived &, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma, Monitor &monitor)
{
    cusp::krylov::cg_m(A, x, b, sigma, monitor);
}
} // namespace policy_default
} // namespace detail

template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3, typename Monitor>
void cg_m(const cusp::execution_policy<Derived> &exec, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma, Monitor &monitor)
{
    using cusp::krylov::detail::policy_default::cg_m;
    cg_m(const_cast<Derived &>(exec.derived()), A, x, b, sigma, monitor);
}
template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3>
void cg_m(const cusp::execution_policy<Derived> &exec, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma)
{
    cusp::monitor<typename LinearOperator::value_type> monitor(b);
    cusp::krylov::cg_m(exec, A, x, b, sigma, monitor);
}

} // namespace krylov
} // namespace cusp
