// cusp/krylov/bicgstab_m.h -- cusp::krylov::bicgstab_m(A, x, b, sigma[, monitor]): multi-shift BiCGstab.  Solves (A + sigma_s I) x_s = b for
// every shift in `sigma` with TWO cusp::multiply per iteration, A non-symmetric (B. Jegerlehner, hep-lat/9612014; reference
// cusp/krylov/bicgstab_m.h, detail/bicgstab_m.inl:697-848 -- the same operations in the same order, in ValueType).  x holds N * N_s values, shift s
// at [s N, (s + 1) N); it is zero-filled on entry.  The monitor watches the residual of the unshifted system.
//
// The scalars of the unshifted system stay on the host, as in the reference: five dots per iteration.  host_memory: plain loops.  device_memory:
// w_1 and r_1 through cusp::blas::axpby (the same bits as KERNEL_W), the rest through cmi_bicgstab_m_s_* / _coefficients_* / _update_xs_*
// (csrc/krylov_m.hip) with the per-shift coefficients in device arrays.
//
// Kept from the reference, not patched: the zeta of a shift that converged long ago can underflow; the clamp then sets 1e-18 and the next
// zeta_0 * zeta_m1 / (...) is 0 / 0 -- that shift's x turns NaN (seen in float on a 33 x 31 Poisson matrix with sigma = 5).
#pragma once
#include <cmath>
#include <type_traits>
#include <vector>

#include "../array1d.h"
#include "../blas/blas.h"
#include "../execution_policy.h"
#include "../monitor.h"
#include "../multiply.h"
#include "cg_m.h"

namespace cusp {
namespace krylov {
namespace detail {
namespace multishift {

// the per-shift state of BiCGstab-M and the three steps that use it, by memory space
template <typename T, typename MemorySpace> struct bicgstab_shifts;

template <typename T> struct bicgstab_shifts<T, cusp::host_memory> {
    std::vector<T> sig, z_m1, z_0, z_1, alpha_s, beta_s, rho_0, rho_1, chi_s;
    template <typename S> explicit bicgstab_shifts(const S &sigma)
        : z_m1(sigma.size(), T(1)), z_0(sigma.size(), T(1)), z_1(sigma.size()), alpha_s(sigma.size(), T(0)), beta_s(sigma.size()), rho_0(sigma.size(), T(1)),
          rho_1(sigma.size()), chi_s(sigma.size())
    {
        const cusp::array1d<T, cusp::host_memory> h(sigma);
        sig.assign(h.begin(), h.end());
    }
    // KERNEL_S
    static void s(size_t N, T alpha_1, T chi_0, const T *r_1, const T *As, T *s_0)
    {
        for (size_t i = 0; i < N; i++) s_0[i] = r_1[i] + alpha_1 * (s_0[i] - chi_0 * As[i]);
    }
    // KERNEL_ZB (+ clamp), KERNEL_CHIRHO, KERNEL_A
    void coefficients(T beta_m1, T beta_0, T alpha_old, T alpha_new, T chi_0)
    {
        for (size_t k = 0; k < sig.size(); k++) {
            zb(beta_m1, beta_0, alpha_old, z_0[k], z_m1[k], sig[k], z_1[k], beta_s[k]);
            const T den = T(1) + chi_0 * sig[k];
            chi_s[k] = chi_0 / den;
            rho_1[k] = rho_0[k] / den;
            alpha_s[k] = a(beta_0, alpha_new, z_0[k], z_1[k], beta_s[k]);
        }
    }
    // KERNEL_XS, then the rotation of zeta and rho
    void update_xs(size_t N, const T *r_0, const T *r_1, const T *w_1, T *x, T *ss)
    {
        for (size_t k = 0; k < sig.size(); k++) {
            const T z1s = z_1[k], b0s = beta_s[k], c0s = chi_s[k];
            for (size_t i = 0; i < N; i++) {
                const T w1 = w_1[i], s_0 = ss[k * N + i];
                x[k * N + i] = x[k * N + i] - b0s * s_0 + c0s * rho_0[k] * z1s * w1;
                ss[k * N + i] = z1s * rho_1[k] * r_1[i] + alpha_s[k] * (s_0 - c0s * rho_0[k] / b0s * (z1s * w1 - z_0[k] * r_0[i]));
            }
        }
        z_m1 = z_0;
        z_0 = z_1;
        rho_0 = rho_1;
    }
};

template <typename T> struct bicgstab_shifts<T, cusp::device_memory> {
    static_assert(cusp::detail::is_real<T>::value, "device_memory bicgstab_m is implemented for float and double");
    typedef cusp::array1d<T, cusp::device_memory> Vec;
    Vec sig, z_m1, z_0, z_1, alpha_s, beta_s, rho_0, rho_1, chi_s;
    template <typename S> explicit bicgstab_shifts(const S &sigma)
        : sig(sigma), z_m1(sigma.size(), T(1)), z_0(sigma.size(), T(1)), z_1(sigma.size()), alpha_s(sigma.size(), T(0)), beta_s(sigma.size()),
          rho_0(sigma.size(), T(1)), rho_1(sigma.size()), chi_s(sigma.size())
    {}
    static void s(size_t N, T alpha_1, T chi_0, const T *r_1, const T *As, T *s_0) { cusp::detail::check(by_type<T>(cmi_bicgstab_m_s_f64, cmi_bicgstab_m_s_f32)(
        N, alpha_1, chi_0, r_1, As, s_0, nullptr)); }
    void coefficients(T beta_m1, T beta_0, T alpha_old, T alpha_new, T chi_0)
    {
        cusp::detail::check(by_type<T>(cmi_bicgstab_m_coefficients_f64, cmi_bicgstab_m_coefficients_f32)(
            sig.size(), beta_m1, beta_0, alpha_old, alpha_new, chi_0, sig.data(), z_m1.data(), z_0.data(), rho_0.data(), z_1.data(),
                                                                                                         beta_s.data(), chi_s.data(), rho_1.data(), alpha_s.data(), nullptr));
    }
    void update_xs(size_t N, const T *r_0, const T *r_1, const T *w_1, T *x, T *ss)
    {
        cusp::detail::check(by_type<T>(cmi_bicgstab_m_update_xs_f64, cmi_bicgstab_m_update_xs_f32)(N, sig.size(), N, beta_s.data(), chi_s.data(), rho_0.data(),
                                                                                                   z_m1.data(), z_0.data(),
                                                                                                   alpha_s.data(), rho_1.data(), z_1.data(), r_0, r_1, w_1, x, ss,
                                                                                                   nullptr)); // (the shifts lie N apart; the rotation rides behind it)
    }
};

} // namespace multishift
} // namespace detail

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3, typename Monitor,
          typename = detail::not_policy<LinearOperator>>
void bicgstab_m(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma, Monitor &monitor)
{
    typedef typename LinearOperator::value_type ValueType;
    typedef typename LinearOperator::memory_space MemorySpace;
    detail::multishift::check_sizes(A, x, b, sigma, "bicgstab_m");
    const size_t N = A.num_rows, N_s = sigma.size();

    cusp::array1d<ValueType, MemorySpace> w_1(N), w_0(N), r_0(N), r_1(N), s_0(N), s_0_s(N * N_s), As(N), Aw(N);
    detail::multishift::bicgstab_shifts<ValueType, MemorySpace> shifts(sigma);
    ValueType beta_m1, beta_0(1), alpha_0(0), delta_0, delta_1, phi_0, chi_0;

    cusp::blas::copy(b, r_0);
    cusp::blas::copy(b, w_1);
    cusp::blas::copy(w_1, w_0);
    cusp::blas::fill(x, ValueType(0));
    detail::multishift::replicate(b.data(), s_0_s.data(), N, N_s, MemorySpace());
    cusp::blas::copy(b, s_0);
    cusp::multiply(A, s_0, As);
    delta_1 = cusp::blas::dotc(w_0, r_0);
    phi_0 = cusp::blas::dotc(w_0, As) / delta_1;

    while (!monitor.finished(r_0)) {
        beta_m1 = beta_0;
        beta_0 = ValueType(-1.0) / phi_0;
        delta_0 = delta_1;
        cusp::blas::axpby(r_0, As, w_1, ValueType(1), beta_0);            // w_1 <- r_0 + beta_0 A s        (KERNEL_W)
        cusp::multiply(A, w_1, Aw);
        chi_0 = cusp::blas::dotc(Aw, w_1) / cusp::blas::dotc(Aw, Aw);
        cusp::blas::axpby(w_1, Aw, r_1, ValueType(1), -chi_0);            // r_1 <- w_1 - chi_0 A w         (KERNEL_W)
        delta_1 = cusp::blas::dotc(w_0, r_1);
        const ValueType alpha_old = alpha_0;
        alpha_0 = -beta_0 * delta_1 / delta_0 / chi_0;
        shifts.s(N, alpha_0, chi_0, r_1.data(), As.data(), s_0.data());   // s_0 <- r_1 + alpha_0 (s_0 - chi_0 A s)
        cusp::multiply(A, s_0, As);
        phi_0 = cusp::blas::dotc(w_0, As) / delta_1;
        shifts.coefficients(beta_m1, beta_0, alpha_old, alpha_0, chi_0);  // zeta_1, beta_s (old alpha); chi_s, rho_1; alpha_s (new alpha)
        shifts.update_xs(N, r_0.data(), r_1.data(), w_1.data(), x.data(), s_0_s.data()); // x_s, s_s; zeta and rho rotate
        cusp::blas::copy(r_1, r_0);
        ++monitor;
    }
}

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3, typename = detail::not_policy<LinearOperator>>
void bicgstab_m(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma)
{
    cusp::monitor<typename LinearOperator::value_type> monitor(b);
    cusp::krylov::bicgstab_m(A, x, b, sigma, monitor);
}

// ---- execution-policy overloads (reference cusp/krylov/bicgstab_m.h): a user `bicgstab_m(my_policy&, ...)` overload is reached by ADL
// (testing/multi_mass.cu:107-148); a policy without one gets the memory-space dispatch above.
namespace detail {
namespace policy_default {
template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3, typename Monitor,
          typename = typename std::enable_if<std::is_base_of<cusp::execution_policy<Derived>, Derived>::value>::type>
void bicgstab_m(Derived &, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma, Monitor &monitor)
{
    cusp::krylov::bicgstab_m(A, x, b, sigma, monitor);
}
template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3,
          typename = typename std::enable_if<std::is_base_of<cusp::execution_policy<Derived>, Derived>::value>::type>
void bicgstab_m(Derived &, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma)
{
    cusp::krylov::bicgstab_m(A, x, b, sigma);
}
} // namespace policy_default
} // namespace detail

template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3, typename Monitor>
void bicgstab_m(const cusp::execution_policy<Derived> &exec, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma, Monitor &monitor)
{
    using cusp::krylov::detail::policy_default::bicgstab_m;
    bicgstab_m(const_cast<Derived &>(exec.derived()), A, x, b, sigma, monitor);
}
template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename VectorType3>
void bicgstab_m(const cusp::execution_policy<Derived> &exec, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, const VectorType3 &sigma)
{
    using cusp::krylov::detail::policy_default::bicgstab_m;
    bicgstab_m(const_cast<Derived &>(exec.derived()), A, x, b, sigma);
}

} // namespace krylov
} // namespace cusp
