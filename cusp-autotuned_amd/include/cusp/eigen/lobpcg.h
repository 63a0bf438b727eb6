// cusp/eigen/lobpcg.h -- cusp::eigen::lobpcg(A, S, X[, monitor[, M]], largest = true): the locally optimal block preconditioned conjugate
// gradient method for ONE extreme eigenpair of a symmetric operator (A. Knyazev, SIAM J. Sci. Comput. 23 (2001); reference cusp/eigen/lobpcg.h,
// detail/lobpcg.inl -- the same operations in the same order).  X (an array1d of A.num_rows values, or an array2d with one column) holds the
// start vector on entry and the Ritz vector on exit; S[0] receives the eigenvalue.  A is any of the five formats or a cusp::linear_operator, M
// any operator cusp::multiply applies, in either memory space.  The loop runs while iteration_count() < min(N, iteration_limit()) and stops
// when ||A x - lambda x|| < monitor.relative_tolerance() -- the tolerance itself, not tolerance(), as in the reference.
//
// Departures from the reference, all deliberate:
//   * Every normalisation multiplies by T(1) / T(norm), formed once in T (cmi_blas_scal_recip_*'s rule); the reference forms 1.0 / norm in
//     double and rounds that, which in float can differ in the last bit.
//   * The 2 x 2 / 3 x 3 Gram problem is solved by cusp/detail/sygv_small.h (Cholesky + Jacobi, no LAPACK).  When it reports that gramB is not
//     positive definite -- the search for the LARGEST eigenvalue in float reaches that -- the Rayleigh-Ritz step is retried once without P
//     (the 2 x 2 pair, c_P = 0); if that fails too the loop stops and lambda, X and the monitor stay as they are (not converged).
//   * The monitor also learns the residual norm (finished_norm), so converged() answers; the reference only appends to monitor.residuals.
//   * The reference's asserts on shapes throw invalid_input_exception.
//
// Two paths:
//   plain  any memory space, any value type: operation by operation through cusp::multiply and cusp::blas (33 vector reads, 9 writes and 12
//          host reads per iteration on device_memory).
//   fused  device_memory, float or double: cmi_blas_scal_recip_* (W = R / ||R|| in place when M is the identity), the multiply,
//          cmi_lobpcg_gram_* (the eight sums, P and AP normalised in the same pass), ONE read of eight doubles, the 3 x 3 problem on the host,
//          cmi_lobpcg_update_* (P, AP, X, AX, R, <R,R>, <P,P>): 12 vector reads, 8 writes and two host reads (the Gram block; ||R|| from
//          the page-locked mirror).  A general M costs one cusp::multiply and one dot more.  $CMI_LOBPCG_FUSED=0 selects the plain path.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "../array1d.h"
#include "../array2d.h"
#include "../blas/blas.h"
#include "../detail/sygv_small.h"
#include "../krylov/cg.h" // pinned_scalar
#include "../linear_operator.h"
#include "../monitor.h"
#include "../multiply.h"

namespace cusp {
namespace eigen {
namespace detail {
namespace lobpcg_detail {

// one Rayleigh-Ritz step: the Gram pair from lambda and the sums g = {<x,aw>, <w,aw>, <x,w>, <x,ap>, <w,ap>, <p,ap>, <x,p>, <w,p>} (the last
// five only with_p), solved in double; the wanted column gives the new lambda and the coefficients of X, W (= R) and P, rounded to T
template <typename T> struct ritz {
    bool ok;     // false: gramB was not positive definite, with and without P -- nothing below is set
    bool used_p; // false: the 2 x 2 pair was solved (the first iteration, or the retry after a 3 x 3 breakdown); cp = 0
    T lambda, cx, cr, cp;
};
template <typename T> ritz<T> ritz_step(T lambda, const T *g, bool with_p, bool largest)
{
    ritz<T> out = {false, false, T(0), T(0), T(0), T(0)};
    for (int n = with_p ? 3 : 2; n >= 2; n--) {
        double A[9], B[9], w[3], Z[9];
        if (n == 3) {
            const double a[9] = {(double)lambda, (double)g[0], (double)g[3], (double)g[0], (double)g[1], (double)g[4], (double)g[3], (double)g[4], (double)g[5]};
            const double b[9] = {1.0, (double)g[2], (double)g[6], (double)g[2], 1.0, (double)g[7], (double)g[6], (double)g[7], 1.0};
            std::copy(a, a + 9, A);
            std::copy(b, b + 9, B);
        } else {
            const double a[4] = {(double)lambda, (double)g[0], (double)g[0], (double)g[1]};
            const double b[4] = {1.0, (double)g[2], (double)g[2], 1.0};
            std::copy(a, a + 4, A);
            std::copy(b, b + 4, B);
        }
        if (!cusp::detail::sygv_small(n, A, B, w, Z)) continue;
        const int col = largest ? n - 1 : 0;
        out.ok = true;
        out.used_p = n == 3;
        out.lambda = static_cast<T>(w[col]);
        out.cx = static_cast<T>(Z[0 * n + col]);
        out.cr = static_cast<T>(Z[1 * n + col]);
        out.cp = n == 3 ? static_cast<T>(Z[2 * n + col]) : T(0);
        return out;
    }
    return out;
}

// X as a vector: an array1d itself, the values of an array2d with one column
template <typename T, typename Space> cusp::array1d<T, Space> &as_vector(cusp::array1d<T, Space> &x) { return x; }
template <typename T, typename Space, typename O> cusp::array1d<T, Space> &as_vector(cusp::array2d<T, Space, O> &x)
{
    if (x.num_cols != 1 || x.values.size() != x.num_rows) throw cusp::invalid_input_exception("lobpcg: X must have one column (and no padding)");
    return x.values;
}

// the residual norm goes to monitor.residuals; a monitor with finished_norm also keeps it, so that converged() can answer
template <typename Monitor> auto note_residual(Monitor &m, typename Monitor::Real norm, int) -> decltype(m.finished_norm(norm), void()) { m.finished_norm(norm); }
template <typename Monitor, typename Real> void note_residual(Monitor &m, Real norm, long) { m.residuals.push_back(norm); }

// reference detail/lobpcg.inl:47-182, operation by operation (any memory space)
template <typename LinearOperator, typename Array1d, typename Vec, typename Monitor, typename Preconditioner>
void lobpcg_plain(const LinearOperator &A, Array1d &S, Vec &X, Monitor &monitor, Preconditioner &M, bool largest)
{
    typedef typename LinearOperator::value_type T;
    const size_t N = A.num_rows;
    cusp::blas::scal(X, T(1) / T(cusp::blas::nrm2(X)));
    Vec AX(N), R(N), P(N, T(0)), AP(N, T(0)), W(N), AW(N);
    cusp::multiply(A, X, AX);
    T lambda = cusp::blas::dot(X, AX);
    while (monitor.iteration_count() < std::min(N, monitor.iteration_limit())) {
        const bool first = monitor.iteration_count() == 0;
        cusp::blas::axpby(X, AX, R, -lambda, T(1));
        const T r_norm = cusp::blas::nrm2(R);
        note_residual(monitor, static_cast<typename Monitor::Real>(r_norm), 0);
        if (r_norm < monitor.relative_tolerance()) break;
        cusp::multiply(M, R, W);
        cusp::blas::scal(W, T(1) / T(cusp::blas::nrm2(W)));
        cusp::multiply(A, W, AW);
        if (!first) {
            const T s = T(1) / T(cusp::blas::nrm2(P));
            cusp::blas::scal(P, s);
            cusp::blas::scal(AP, s);
        }
        T g[8] = {cusp::blas::dot(X, AW), cusp::blas::dot(W, AW), cusp::blas::dot(X, W), T(0), T(0), T(0), T(0), T(0)};
        if (!first) {
            g[3] = cusp::blas::dot(X, AP);
            g[4] = cusp::blas::dot(W, AP);
            g[5] = cusp::blas::dot(P, AP);
            g[6] = cusp::blas::dot(X, P);
            g[7] = cusp::blas::dot(W, P);
        }
        const ritz<T> z = ritz_step(lambda, g, !first, largest);
        if (!z.ok) break; // gramB is not positive definite: lambda, X and the monitor stay as they are
        lambda = z.lambda;
        if (first) {
            cusp::blas::axpy(W, P, z.cr);
            cusp::blas::axpy(AW, AP, z.cr);
        } else {
            cusp::blas::axpby(W, P, P, z.cr, z.cp);
            cusp::blas::axpby(AW, AP, AP, z.cr, z.cp);
        }
        cusp::blas::axpby(X, P, X, z.cx, T(1));
        cusp::blas::axpby(AX, AP, AX, z.cx, T(1));
        ++monitor;
    }
    S[0] = lambda;
}

// device_memory, float / double: the schedule at the head of this file
template <typename LinearOperator, typename Array1d, typename Vec, typename Monitor, typename Preconditioner>
void lobpcg_fused_device(const LinearOperator &A, Array1d &S, Vec &X, Monitor &monitor, Preconditioner &M, bool largest)
{
    typedef typename LinearOperator::value_type T;
    using cusp::detail::by_type;
    using cusp::detail::check;
    constexpr bool identity_m = std::is_same<typename std::remove_const<Preconditioner>::type, cusp::identity_operator<T, cusp::device_memory>>::value;
    const size_t N = A.num_rows;
    Vec AX(N), Ra(N), Rb(N), P(N, T(0)), AP(N, T(0)), AW(N);
    cusp::array1d<double, cusp::device_memory> scalars(12); // [0] <r,r>  [1] <p,p>  [2] lambda at the start, <w,w>  [4..11] the Gram sums
    double *rr = scalars.data(), *pp = rr + 1, *tmp = rr + 2, *gram = rr + 4;
    cusp::blas::detail::device_workspace &ws = cusp::blas::detail::workspace();
    cusp::krylov::detail::pinned_scalar rr_host;
    check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, X.data(), X.data(), tmp, ws.ws, nullptr));
    check(by_type<T>(cmi_blas_scal_recip_f64, cmi_blas_scal_recip_f32)(N, tmp, 1, X.data(), nullptr, nullptr));
    cusp::multiply(A, X, AX);
    check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, X.data(), AX.data(), tmp, ws.ws, nullptr));
    Vec *r = &Ra, *other = &Rb;
    check(by_type<T>(cmi_lobpcg_residual_f64, cmi_lobpcg_residual_f32)(N, tmp, X.data(), AX.data(), r->data(), rr, rr_host.host, ws.ws, nullptr));
    rr_host.record();
    double lambda_d;
    check(cmi_memcpy_d2h(&lambda_d, tmp, sizeof(double), nullptr));
    T lambda = static_cast<T>(lambda_d);
    while (monitor.iteration_count() < std::min(N, monitor.iteration_limit())) {
        const bool first = monitor.iteration_count() == 0;
        const T r_norm = static_cast<T>(std::sqrt(rr_host.wait())); // host read: ||r||
        note_residual(monitor, static_cast<typename Monitor::Real>(r_norm), 0);
        if (r_norm < monitor.relative_tolerance()) break;
        Vec *w, *r_next;
        if constexpr (identity_m) { // W = R / ||R|| in place; the new residual goes to the other buffer
            check(by_type<T>(cmi_blas_scal_recip_f64, cmi_blas_scal_recip_f32)(N, rr, 1, r->data(), nullptr, nullptr));
            w = r;
            r_next = other;
        } else {
            cusp::multiply(M, *r, *other);
            check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, other->data(), other->data(), tmp, ws.ws, nullptr));
            check(by_type<T>(cmi_blas_scal_recip_f64, cmi_blas_scal_recip_f32)(N, tmp, 1, other->data(), nullptr, nullptr));
            w = other;
            r_next = r;
        }
        cusp::multiply(A, *w, AW);
        check(by_type<T>(cmi_lobpcg_gram_f64, cmi_lobpcg_gram_f32)(N, first ? nullptr : pp, X.data(), w->data(), AW.data(), first ? nullptr : P.data(),
                                                                   first ? nullptr : AP.data(), gram, ws.ws, nullptr));
        double gd[8] = {};
        check(cmi_memcpy_d2h(gd, gram, (first ? 3 : 8) * sizeof(double), nullptr)); // host read: the Gram block
        T g[8];
        for (int k = 0; k < 8; k++) g[k] = static_cast<T>(gd[k]);
        const ritz<T> z = ritz_step(lambda, g, !first, largest);
        if (!z.ok) break;
        lambda = z.lambda;
        // a 2 x 2 retry behind a scaled P: cp = 0 drops it, as the plain path's axpby does
        check(by_type<T>(cmi_lobpcg_update_f64, cmi_lobpcg_update_f32)(N, z.cx, z.cr, z.cp, first ? 1 : 0, lambda, w->data(), AW.data(), P.data(), AP.data(), X.data(),
                                                                       AX.data(), r_next->data(), rr, rr_host.host, ws.ws, nullptr));
        rr_host.record();
        if constexpr (identity_m) std::swap(r, other);
        ++monitor;
    }
    check(cmi_device_synchronize()); // nothing queued may outlive the temporaries
    S[0] = lambda;
}

template <typename A, typename S, typename X> void check_shapes(const A &a, const S &s, const X &x)
{
    if (a.num_rows != a.num_cols) throw cusp::invalid_input_exception("lobpcg: matrix must be square");
    if (x.size() != a.num_rows) throw cusp::invalid_input_exception("lobpcg: X must hold num_rows values");
    if (s.size() < 1) throw cusp::invalid_input_exception("lobpcg: S must hold at least one value");
}

template <typename M> struct is_monitor : std::integral_constant<bool, !std::is_arithmetic<M>::value> {};

} // namespace lobpcg_detail
} // namespace detail

template <typename LinearOperator, typename Array1d, typename Array2d, typename Monitor, typename Preconditioner,
          typename = typename std::enable_if<detail::lobpcg_detail::is_monitor<Monitor>::value && !std::is_arithmetic<Preconditioner>::value>::type>
void lobpcg(const LinearOperator &A, Array1d &S, Array2d &X, Monitor &monitor, Preconditioner &M, bool largest = true)
{
    namespace d = detail::lobpcg_detail;
    typedef typename LinearOperator::value_type T;
    auto &x = d::as_vector(X);
    d::check_shapes(A, S, x);
    typedef typename std::remove_reference<decltype(x)>::type Vec;
    if constexpr (std::is_same<typename LinearOperator::memory_space, cusp::device_memory>::value && cusp::detail::is_real<T>::value &&
                  std::is_same<typename Vec::value_type, T>::value && std::is_same<typename Vec::memory_space, cusp::device_memory>::value) {
        const char *e = std::getenv("CMI_LOBPCG_FUSED");
        if (e && e[0] == '0') d::lobpcg_plain(A, S, x, monitor, M, largest); // (measurements: the operation-by-operation path)
        else d::lobpcg_fused_device(A, S, x, monitor, M, largest);
    } else {
        d::lobpcg_plain(A, S, x, monitor, M, largest);
    }
}

template <typename LinearOperator, typename Array1d, typename Array2d, typename Monitor,
          typename = typename std::enable_if<detail::lobpcg_detail::is_monitor<Monitor>::value>::type>
void lobpcg(const LinearOperator &A, Array1d &S, Array2d &X, Monitor &monitor, bool largest = true)
{
    typedef typename LinearOperator::value_type T;
    typedef typename LinearOperator::memory_space MemorySpace;
    cusp::identity_operator<T, MemorySpace> M(A.num_rows, A.num_cols);
    cusp::eigen::lobpcg(A, S, X, monitor, M, largest);
}

template <typename LinearOperator, typename Array1d, typename Array2d> void lobpcg(const LinearOperator &A, Array1d &S, Array2d &X, bool largest = true)
{
    typedef typename LinearOperator::value_type T;
    const cusp::array1d<T, cusp::host_memory> b(A.num_rows, T(1)); // the reference's constant_array of ones: the default monitor (500, 1e-5)
    cusp::monitor<T> monitor(b);
    cusp::eigen::lobpcg(A, S, X, monitor, largest);
}

} // namespace eigen
} // namespace cusp
