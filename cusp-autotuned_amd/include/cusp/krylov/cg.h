// cusp/krylov/cg.h -- (preconditioned) conjugate gradients, the caller of the SpMV hot path
// (reference cusp/krylov/cg.h, cusp/krylov/detail/cg.inl:41-107: same operations in the same order,
// so the residual history matches the reference's, e.g. docs/quickstart.md:72-87).
// One cusp::multiply per iteration -> cmi_spmv_* on device_memory; vector updates -> cusp::blas.
#pragma once
#include <cassert>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "../array1d.h"
#include "../blas/blas.h"
#include "../execution_policy.h"
#include "../linear_operator.h"
#include "../monitor.h"
#include "../multiply.h"
#include "detail/multiply_dot.h"

namespace cusp {
namespace precond {
template <typename ValueType, typename MemorySpace> class diagonal;
template <typename ValueType, typename MemorySpace> class scaled_bridson_ainv;
template <typename ValueType, typename MemorySpace> class bridson_ainv;
template <typename ValueType, typename MemorySpace> class nonsym_bridson_ainv;
} // namespace precond
namespace krylov {

namespace detail {
// the overloads without a policy must not swallow cg(policy, A, x, b[, monitor]) calls
template <typename T> struct is_policy : std::is_base_of<cusp::execution_policy<T>, T> {};
// (the solvers skip the copy an identity preconditioner would make)
template <typename M> struct is_identity : std::false_type {};
template <typename V, typename S, typename I> struct is_identity<cusp::identity_operator<V, S, I>> : std::true_type {};
template <typename V, typename S, typename I> struct is_identity<const cusp::identity_operator<V, S, I>> : std::true_type {};
template <typename T> using not_policy = typename std::enable_if<!is_policy<T>::value>::type;
// the approximate-inverse preconditioners of cusp/precond/ainv.h on device_memory with the solver's value type (cg's fused branch for them)
template <typename M, typename T> struct is_device_ainv : std::false_type {};
template <typename T> struct is_device_ainv<cusp::precond::scaled_bridson_ainv<T, cusp::device_memory>, T> : std::true_type {};
template <typename T> struct is_device_ainv<cusp::precond::bridson_ainv<T, cusp::device_memory>, T> : std::true_type {};
template <typename T> struct is_device_ainv<cusp::precond::nonsym_bridson_ainv<T, cusp::device_memory>, T> : std::true_type {};

// z <- M r for a matrix-like preconditioner or a linear operator with operator()
template <typename M, typename X, typename Y> auto apply(const M &m, const X &x, Y &y, int) -> decltype(m(x, y), void()) { m(x, y); }
template <typename M, typename X, typename Y> void apply(const M &m, const X &x, Y &y, long) { cusp::multiply(m, x, y); }
} // namespace detail

namespace detail {

// Fused unpreconditioned CG on the device (f64 and f32): z == r is folded away, alpha and beta stay in device
// memory, and an iteration is
//     cmi_spmv_csr_dot_f64 (y <- A p and <y,p> in one pass; the ladder of detail/multiply_dot.h)
//     cmi_cg_update_f64      (r, <r,r> in one pass)
//     cmi_cg_direction_x_f64 (x <- x + alpha p, p <- r + beta p in one pass)
// i.e. 3 launches, 8 vector passes and ONE host read (the convergence check) instead of cg.inl's 7 passes and 3 host syncs.
// The host read needs no copy: cmi_cg_update's reduction also writes <r,r> into page-locked host
// memory, and the host waits for the event behind it only AFTER it has queued the next iteration's SpMV (which reads p and writes the scratch y -- no solver state -- so
// running it speculatively is harmless if the monitor then stops), so the device never idles on the
// round trip.  Per-element arithmetic unchanged; the residual history agrees with the plain path to
// rounding.
template <typename Monitor> auto has_finished_norm(Monitor *m) -> decltype(m->finished_norm(typename Monitor::Real()), std::true_type());
std::false_type has_finished_norm(...);
// what every fused iteration needs: device_memory, float or double, x of the matrix's value type, a monitor that takes the norm itself
template <typename A, typename X, typename Monitor> struct fused_eligible {
    typedef typename A::value_type T;
    static const bool value = std::is_same<typename A::memory_space, cusp::device_memory>::value && cusp::detail::is_real<T>::value &&
                              std::is_same<typename X::value_type, T>::value && decltype(has_finished_norm(static_cast<Monitor *>(nullptr)))::value;
};

struct pinned_scalar { // 8 page-locked bytes + the event that says they have landed
    double *host;
    void *event;
    pinned_scalar() : host(nullptr), event(nullptr)
    {
        void *h = nullptr;
        cusp::detail::check(cmi_malloc_host(&h, sizeof(double)));
        host = static_cast<double *>(h);
        const int st = cmi_event_create(&event);
        if (st != CMI_SUCCESS) { cmi_free_host(host); cusp::detail::check(st); }
    }
    ~pinned_scalar() { if (event) cmi_event_destroy(event); if (host) cmi_free_host(host); }
    pinned_scalar(const pinned_scalar &) = delete;
    pinned_scalar &operator=(const pinned_scalar &) = delete;
    void fetch(const double *dev) // queue the copy; returns at once
    {
        cusp::detail::check(cmi_memcpy_d2h_async(host, dev, sizeof(double), nullptr));
        record();
    }
    void record() { cusp::detail::check(cmi_event_record(event, nullptr)); } // behind a kernel that wrote *host itself
    double wait() { cusp::detail::check(cmi_event_synchronize(event)); return *host; }
};

// Fold-ahead form (CSR through its plan): the SpMV leaves the per-tile partials of <y, p> in the workspace and the update
// kernel folds them itself; likewise <r, r> is folded at the front of the direction kernel -- no fold launches in between
// (cmi_cg_update_fold_*, cusp_mi355x.h); opt-in, see fold_ahead_enabled().  Returns the partial count, 0 when this operator / plan
// cannot (then *yp is not set).
inline bool fold_ahead_enabled()
{
    // opt-in ($CMI_CG_FOLD_AHEAD=1): measured 268.8 vs 272.7 us per iteration on the headline matrix (-1.4 %), 252.5 vs 254.0
    // with the 16-bit column copy -- inside the box-to-box spread, so the default stays the five-launch iteration, which has
    // no workgroup waiting on another
    static const bool on = [] { const char *e = std::getenv("CMI_CG_FOLD_AHEAD"); return e && e[0] == '1'; }();
    return on;
}
template <typename A, typename V> int multiply_dot_partials(const A &a, const V &p, V &y, void *ws, cusp::csr_format)
{
    cusp::detail::require_int_index<A>();
    if (!fold_ahead_enabled() || p.size() != a.num_cols || y.size() != a.num_rows) return 0;
    const cmi_plan *pl = cusp::detail::plan_of(a, nullptr, 0);
    if (!pl) return 0;
    int np = 0;
    cusp::detail::check(by_type<typename A::value_type>(cmi_spmv_csr_dot_plan_partials_f64, cmi_spmv_csr_dot_plan_partials_f32)(
        pl, a.row_offsets.data(), a.column_indices.data(), a.values.data(), p.data(), y.data(), p.data(), ws, &np, nullptr));
    if (np > 0) return np;
    return -1; // y is computed, but this plan's kernel left no partials: the caller adds the separate dot
}
template <typename A, typename V, typename Format> int multiply_dot_partials(const A &, const V &, V &, void *, Format) { return 0; }
template <typename A, typename V> int multiply_dot_partials_any(const A &a, const V &p, V &y, void *ws)
{
    if constexpr (cusp::detail::has_format<A>::value) return multiply_dot_partials(a, p, y, ws, typename A::format());
    else return 0;
}

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor>
void cg_fused_device(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor)
{
    typedef typename LinearOperator::value_type T;
    const size_t N = A.num_rows;
    cusp::array1d<T, cusp::device_memory> y(N), r(N), p(N);
    cusp::array1d<double, cusp::device_memory> scalars(3); // rr[0], rr[1], <y,p>
    cusp::blas::detail::device_workspace &w = cusp::blas::detail::workspace();
    double *rr[2] = {scalars.data(), scalars.data() + 1};
    double *yp = scalars.data() + 2;
    pinned_scalar rr_host;
    cusp::multiply(A, x, y);
    cusp::blas::axpby(b, y, r, T(1), T(-1));
    cusp::blas::copy(r, p);
    cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, r.data(), r.data(), rr[0], w.ws, nullptr));
    rr_host.fetch(rr[0]);
    int cur = 0;
    for (;;) {
        // the hot path (speculative, see above).  CSR through its plan: the partials of <y, p> stay in the workspace (np > 0)
        int np = multiply_dot_partials_any(A, p, y, w.ws);
        if (np == 0) multiply_dot(A, p, y, p, yp, w.ws);
        else if (np < 0) { cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, y.data(), p.data(), yp, w.ws, nullptr)); np = 0; }
        if (monitor.finished_norm(static_cast<typename Monitor::Real>(std::sqrt(rr_host.wait())))) break; // the one host read
        if (np > 0) { // fold-ahead: three launches per iteration, the two folds ride at the front of their consumers
            int np_rr = 0;
            cusp::detail::check(by_type<T>(cmi_cg_update_fold_f64, cmi_cg_update_fold_f32)(N, rr[cur], yp, np, y.data(), r.data(), w.ws, &np_rr, nullptr));
            cusp::detail::check(by_type<T>(cmi_cg_direction_x_fold_f64, cmi_cg_direction_x_fold_f32)(
                N, rr[cur ^ 1], rr_host.host, np_rr, rr[cur], yp, r.data(), p.data(), x.data(), w.ws,
                                                                                                     nullptr));
            rr_host.record();
        } else {
            cusp::detail::check(by_type<T>(cmi_cg_update_f64, cmi_cg_update_f32)(N, rr[cur], yp, nullptr, y.data(), nullptr, r.data(), rr[cur ^ 1], rr_host.host, w.ws, nullptr));
            rr_host.record();
            // x <- x + alpha p rides with the direction pass (it reads p anyway): 8 vector passes per iteration, not 9
            cusp::detail::check(by_type<T>(cmi_cg_direction_x_f64, cmi_cg_direction_x_f32)(N, rr[cur ^ 1], rr[cur], yp, r.data(), p.data(), x.data(), nullptr));
        }
        cur ^= 1;
        ++monitor;
    }
    cusp::detail::check(cmi_device_synchronize()); // the discarded SpMV must not outlive y
}

// M = cusp::precond::diagonal on device_memory: the same schedule with z = D^-1 r never stored (cmi_pcg_update_jacobi_* / cmi_pcg_direction_x_jacobi_*):
// SpMV + <y,p>, the update with BOTH <r,z> (for alpha / beta) and <r,r> (for the monitor, as the reference's monitor.finished(r)), the direction
// pass -- one host read per iteration behind the next, speculative multiply.
template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename Diagonal>
void cg_fused_jacobi_device(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor, const Diagonal &M)
{
    typedef typename LinearOperator::value_type T;
    const size_t N = A.num_rows;
    const T *dinv = M.reciprocals().data();
    cusp::array1d<T, cusp::device_memory> y(N), r(N), p(N);
    cusp::array1d<double, cusp::device_memory> scalars(4); // <r,z>[0], <r,z>[1], <y,p>, <r,r>
    cusp::blas::detail::device_workspace &w = cusp::blas::detail::workspace();
    double *rz[2] = {scalars.data(), scalars.data() + 1};
    double *yp = scalars.data() + 2, *rr = scalars.data() + 3;
    pinned_scalar rr_host;
    cusp::multiply(A, x, y);
    cusp::blas::axpby(b, y, r, T(1), T(-1));
    cusp::blas::xmy(M.reciprocals(), r, p);                           // p <- z = D^-1 r
    cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, r.data(), p.data(), rz[0], w.ws, nullptr)); // <r, z>
    cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, r.data(), r.data(), rr, w.ws, nullptr));
    rr_host.fetch(rr);
    int cur = 0;
    for (;;) {
        multiply_dot(A, p, y, p, yp, w.ws); // the hot path, speculative: y <- A p, *yp <- <y, p>
        if (monitor.finished_norm(static_cast<typename Monitor::Real>(std::sqrt(rr_host.wait())))) break; // the one host read
        cusp::detail::check(by_type<T>(cmi_pcg_update_jacobi_f64, cmi_pcg_update_jacobi_f32)(N, rz[cur], yp, y.data(), r.data(), dinv, rz[cur ^ 1], rr, rr_host.host,
                                                                                             w.ws, nullptr));
        rr_host.record();
        cusp::detail::check(by_type<T>(cmi_pcg_direction_x_jacobi_f64, cmi_pcg_direction_x_jacobi_f32)(N, rz[cur ^ 1], rz[cur], yp, r.data(), dinv, p.data(), x.data(), nullptr));
        cur ^= 1;
        ++monitor;
    }
    cusp::detail::check(cmi_device_synchronize()); // the discarded SpMV must not outlive y
}

// M = one of the approximate-inverse preconditioners (cusp/precond/ainv.h) on device_memory: the same schedule with z STORED.  The update is
// cmi_cg_update_* with x == NULL and <r,z> in the numerator slot (r <- r - alpha y and <r,r> for the monitor, into the pinned mirror); the apply's
// last multiply is multiply_dot(w_t, t, z, r, <r,z>), so <r,z> costs no launch; cmi_cg_direction_x_* takes z in the slot of r (x <- x + alpha p,
// p <- z + beta p).  Five launches (SpMV + dot, update, the apply's two multiplies, direction) and one host read per iteration, against cg_plain's
// operation by operation with three host reads.  No new vector kernel: the existing ones take these operands as pointers.
template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename Ainv>
void cg_fused_ainv_device(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor, const Ainv &M)
{
    typedef typename LinearOperator::value_type T;
    const size_t N = A.num_rows;
    cusp::array1d<T, cusp::device_memory> y(N), r(N), p(N), z(N);
    cusp::array1d<double, cusp::device_memory> scalars(4); // <r,z>[0], <r,z>[1], <y,p>, <r,r>
    cusp::blas::detail::device_workspace &w = cusp::blas::detail::workspace();
    double *rz[2] = {scalars.data(), scalars.data() + 1};
    double *yp = scalars.data() + 2, *rr = scalars.data() + 3;
    pinned_scalar rr_host;
    cusp::multiply(A, x, y);
    cusp::blas::axpby(b, y, r, T(1), T(-1));
    M.apply_dot(r, z, rz[0], w.ws);                                   // z <- M r, <r, z>
    cusp::blas::copy(z, p);
    cusp::detail::check(by_type<T>(cmi_blas_dot_f64, cmi_blas_dotd_f32)(N, r.data(), r.data(), rr, w.ws, nullptr));
    rr_host.fetch(rr);
    int cur = 0;
    for (;;) {
        multiply_dot(A, p, y, p, yp, w.ws); // the hot path, speculative: y <- A p, *yp <- <y, p>
        if (monitor.finished_norm(static_cast<typename Monitor::Real>(std::sqrt(rr_host.wait())))) break; // the one host read
        cusp::detail::check(by_type<T>(cmi_cg_update_f64, cmi_cg_update_f32)(N, rz[cur], yp, nullptr, y.data(), nullptr, r.data(), rr, rr_host.host, w.ws, nullptr));
        rr_host.record();
        M.apply_dot(r, z, rz[cur ^ 1], w.ws);
        cusp::detail::check(by_type<T>(cmi_cg_direction_x_f64, cmi_cg_direction_x_f32)(N, rz[cur ^ 1], rz[cur], yp, z.data(), p.data(), x.data(), nullptr));
        cur ^= 1;
        ++monitor;
    }
    cusp::detail::check(cmi_device_synchronize()); // the discarded SpMV must not outlive y
}

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename Preconditioner>
void cg_plain(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor, Preconditioner &M);

} // namespace detail

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename Preconditioner,
          typename = detail::not_policy<LinearOperator>>
void cg(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor, Preconditioner &M)
{
    if (A.num_rows != A.num_cols) throw cusp::invalid_input_exception("cg: matrix must be square");
    typedef typename LinearOperator::value_type T;
    constexpr bool eligible = detail::fused_eligible<LinearOperator, VectorType1, Monitor>::value;
    if constexpr (eligible && std::is_same<Preconditioner, cusp::identity_operator<T, cusp::device_memory>>::value) {
        detail::cg_fused_device(A, x, b, monitor);
    } else if constexpr (eligible && std::is_same<typename std::remove_const<Preconditioner>::type, cusp::precond::diagonal<T, cusp::device_memory>>::value) {
        const char *e = std::getenv("CMI_CG_FUSED_JACOBI");
        if (e && e[0] == '0') detail::cg_plain(A, x, b, monitor, M); // (measurements: the operation-by-operation path)
        else detail::cg_fused_jacobi_device(A, x, b, monitor, M);
    } else if constexpr (eligible && detail::is_device_ainv<typename std::remove_const<Preconditioner>::type, T>::value) {
        const char *e = std::getenv("CMI_CG_FUSED_AINV");
        if (e && e[0] == '0') detail::cg_plain(A, x, b, monitor, M); // (measurements and tests: the operation-by-operation path)
        else detail::cg_fused_ainv_device(A, x, b, monitor, M);
    } else {
        detail::cg_plain(A, x, b, monitor, M);
    }
}

// reference cusp/krylov/detail/cg.inl:41-107, operation by operation (any memory space, any M)
template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename Preconditioner>
void detail::cg_plain(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor, Preconditioner &M)
{
    typedef typename LinearOperator::value_type ValueType;
    typedef typename LinearOperator::memory_space MemorySpace;
    const size_t N = A.num_rows;

    // workspace (reference: four temporary_array's, cg.inl:55-58)
    cusp::array1d<ValueType, MemorySpace> y(N), z(N), r(N), p(N);

    cusp::multiply(A, x, y);                                   // y <- A x
    cusp::blas::axpby(b, y, r, ValueType(1), ValueType(-1));   // r <- b - A x
    detail::apply(M, r, z, 0);                                 // z <- M r
    cusp::blas::copy(z, p);                                    // p <- z
    ValueType rz = cusp::blas::dotc(r, z);                     // rz = <r, z>

    while (!monitor.finished(r)) {
        cusp::multiply(A, p, y);                               // y <- A p          (the hot path)
        const ValueType alpha = rz / cusp::blas::dotc(y, p);   // alpha <- <r,z>/<y,p>
        cusp::blas::axpy(p, x, alpha);                         // x <- x + alpha p
        cusp::blas::axpy(y, r, -alpha);                        // r <- r - alpha y
        detail::apply(M, r, z, 0);                             // z <- M r
        const ValueType rz_old = rz;
        rz = cusp::blas::dotc(r, z);
        const ValueType beta = rz / rz_old;
        cusp::blas::axpby(z, p, p, ValueType(1), beta);        // p <- z + beta p
        ++monitor;
    }
}

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename = detail::not_policy<LinearOperator>>
void cg(const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor)
{
    typedef typename LinearOperator::value_type ValueType;
    typedef typename LinearOperator::memory_space MemorySpace;
    cusp::identity_operator<ValueType, MemorySpace> M(A.num_rows, A.num_cols);
    cusp::krylov::cg(A, x, b, monitor, M);
}

template <typename LinearOperator, typename VectorType1, typename VectorType2, typename = detail::not_policy<LinearOperator>>
void cg(const LinearOperator &A, VectorType1 &x, const VectorType2 &b)
{
    typedef typename LinearOperator::value_type ValueType;
    cusp::monitor<ValueType> monitor(b);
    cusp::krylov::cg(A, x, b, monitor);
}

} // namespace krylov
} // namespace cusp

// ---- execution-policy overloads (reference cusp/krylov/cg.h: cg(exec, A, x, b[, monitor[, M]])) ---------
// A policy derived from cusp::execution_policy<Derived> reaches a user `cg(my_policy&, ...)` overload by ADL
// (testing/cg.cu:11-44); a policy without one gets the memory-space dispatch above.
namespace cusp {
namespace krylov {
namespace detail {
namespace policy_default {
template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename Preconditioner,
          typename = typename std::enable_if<std::is_base_of<cusp::execution_policy<Derived>, Derived>::value>::type>
void cg(Derived &, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor, Preconditioner &M)
{
    cusp::krylov::cg(A, x, b, monitor, M);
}
} // namespace policy_default
} // namespace detail

template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor, typename Preconditioner>
void cg(const cusp::execution_policy<Derived> &exec, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor, Preconditioner &M)
{
    using cusp::krylov::detail::policy_default::cg;
    cg(const_cast<Derived &>(exec.derived()), A, x, b, monitor, M);
}
template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2, typename Monitor>
void cg(const cusp::execution_policy<Derived> &exec, const LinearOperator &A, VectorType1 &x, const VectorType2 &b, Monitor &monitor)
{
    typedef typename LinearOperator::value_type ValueType;
    typedef typename LinearOperator::memory_space MemorySpace;
    cusp::identity_operator<ValueType, MemorySpace> M(A.num_rows, A.num_cols);
    cusp::krylov::cg(exec, A, x, b, monitor, M);
}
template <typename Derived, typename LinearOperator, typename VectorType1, typename VectorType2>
void cg(const cusp::execution_policy<Derived> &exec, const LinearOperator &A, VectorType1 &x, const VectorType2 &b)
{
    typedef typename LinearOperator::value_type ValueType;
    cusp::monitor<ValueType> monitor(b);
    cusp::krylov::cg(exec, A, x, b, monitor);
}
} // namespace krylov
} // namespace cusp
