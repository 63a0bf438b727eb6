// cusp/eigen/arnoldi.h -- cusp::eigen::arnoldi(A, H, k): k steps of the Arnoldi process from a random start; H receives the square upper
// Hessenberg matrix of the orthogonalisation coefficients (reference cusp/eigen/arnoldi.h, detail/arnoldi.inl: the same loop -- the start is
// cusp::random_array<ValueType>(N), normalised; modified Gram-Schmidt against the basis one vector at a time; breakdown below 1e-10).
// detail::lanczos_estimate(A, H, k) is the three-term form for symmetric operators (reference detail/spectral_radius.inl).
// A is any of the five formats or a cusp::linear_operator with operator()(x, y), in either memory space; H a host array2d.
//
//   host_memory, and device_memory with a value type other than float / double: the reference's sequence through cusp::multiply and
//                   cusp::blas, one operation and -- on the device -- one host read at a time.
//   device_memory, float / double: no operation-by-operation host reads.  Step j is ONE multiply (a container: through its plan), the chain of
//                   fused Gram-Schmidt steps cusp::krylov::gmres uses (cmi_blas_axpy_dot_*: the axpy of basis vector i and the dot with vector i + 1
//                   in one pass, the coefficients in device memory; j + 2 launches: the first dot has no axpy in front of it, the last axpy
//                   carries the norm's square) and ONE normalise launch that takes the norm from device memory (cmi_blas_scal_recip_*).  The
//                   normalise launch is enqueued BEFORE the step's one host read -- the column of H and beta together -- so the device
//                   does not idle while the host decides; on breakdown the vector it scaled is never used again.  A Lanczos step is the
//                   multiply, two fused launches and the normalise launch, which also leaves beta in device memory for the next step.
//
// ONE DELIBERATE DEPARTURE FROM THE REFERENCE.  On breakdown at step j (beta < 1e-10) the reference returns the leading j x j block: it drops
// column j, which is complete at that point (all of H(0..j, j) is computed; only the vector j + 1 does not exist).  A 2 x 2 diagonal matrix
// breaks down at j = 1 and then yields a 1 x 1 block: the Rayleigh quotient of the random start -- for diag(-5, 2) relative errors up to
// 0.99.  Here the completed column is kept: the block is (j + 1) x (j + 1), both in arnoldi and in lanczos_estimate, and diag(-5, 2) gives 5.
// Without breakdown the result is the reference's k x k block.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "../array1d.h"
#include "../array2d.h"
#include "../blas/blas.h"
#include "../copy.h"
#include "../multiply.h"

namespace cusp {
namespace eigen {
namespace detail {

// the fused device sequence: device_memory and float / double (the index type plays no part: A is only ever multiplied)
template <typename Matrix> struct fused_on_device {
    typedef typename Matrix::value_type V;
    static const bool value = std::is_same<typename Matrix::memory_space, cusp::device_memory>::value && (std::is_same<V, double>::value || std::is_same<V, float>::value);
};

// `count` doubles of device memory for the coefficients of one step, kept per thread between calls (as gmres keeps its own)
inline double *device_coefficients(size_t count)
{
    static thread_local cusp::array1d<double, cusp::device_memory> c;
    if (c.size() < count) c.resize(count + 32);
    return c.data();
}
// x <- x / ||x||_2 with the norm in device memory (c[0] receives its square)
template <typename Vec> void normalize_on_device(Vec &x, double *c, void *ws)
{
    typedef typename Vec::value_type T;
    cusp::detail::check(cusp::detail::by_type<T>(cmi_blas_axpy_dot_f64, cmi_blas_axpy_dot_f32)(x.size(), nullptr, x.data(), x.data(), x.data(), c, ws, nullptr));
    cusp::detail::check(cusp::detail::by_type<T>(cmi_blas_scal_recip_f64, cmi_blas_scal_recip_f32)(x.size(), c, 1, x.data(), nullptr, nullptr));
}

// the leading `size` x `size` block of H_ (size = steps taken, breakdown step included: see the head of this file)
template <typename Work, typename Array2d> void leading_block(const Work &H_, Array2d &H, size_t size)
{
    H.resize(size, size);
    for (size_t row = 0; row < size; row++)
        for (size_t col = 0; col < size; col++) H(row, col) = H_(row, col);
}

template <typename Matrix, typename Array2d> void arnoldi(const Matrix &A, Array2d &H, size_t k, std::false_type)
{
    typedef typename Matrix::value_type ValueType;
    typedef typename Matrix::memory_space MemorySpace;
    const size_t N = A.num_rows, maxiter = std::min(N, k);
    cusp::array2d<ValueType, cusp::host_memory> H_(maxiter + 1, maxiter, ValueType(0));
    std::vector<cusp::array1d<ValueType, MemorySpace>> V(maxiter + 1);
    for (size_t i = 0; i < maxiter + 1; i++) V[i].resize(N);
    cusp::copy(cusp::random_array<ValueType>(N), V[0]);
    cusp::blas::scal(V[0], ValueType(1) / cusp::blas::nrm2(V[0]));
    size_t j;
    for (j = 0; j < maxiter; j++) {
        cusp::multiply(A, V[j], V[j + 1]);
        for (size_t i = 0; i <= j; i++) {
            H_(i, j) = cusp::blas::dotc(V[i], V[j + 1]);
            cusp::blas::axpy(V[i], V[j + 1], -H_(i, j));
        }
        const ValueType beta = cusp::blas::nrm2(V[j + 1]);
        H_(j + 1, j) = beta;
        if (beta < 1e-10) { j++; break; } // column j is complete: it stays
        cusp::blas::scal(V[j + 1], ValueType(1) / H_(j + 1, j));
    }
    leading_block(H_, H, j);
}

template <typename Matrix, typename Array2d> void arnoldi(const Matrix &A, Array2d &H, size_t k, std::true_type)
{
    typedef typename Matrix::value_type ValueType;
    const size_t N = A.num_rows, maxiter = std::min(N, k);
    cusp::array2d<ValueType, cusp::host_memory> H_(maxiter + 1, maxiter, ValueType(0));
    std::vector<cusp::array1d<ValueType, cusp::device_memory>> V(maxiter + 1);
    for (size_t i = 0; i < maxiter + 1; i++) V[i].resize(N);
    if (N == 0) { leading_block(H_, H, 0); return; }
    cusp::blas::detail::device_workspace &ws = cusp::blas::detail::workspace();
    double *c = device_coefficients(maxiter + 2);
    std::vector<double> host(maxiter + 2);
    cusp::copy(cusp::random_array<ValueType>(N), V[0]);
    normalize_on_device(V[0], c, ws.ws);
    size_t j;
    for (j = 0; j < maxiter; j++) {
        ValueType *w = V[j + 1].data();
        cusp::multiply(A, V[j], V[j + 1]);
        cusp::detail::check(cusp::detail::by_type<ValueType>(cmi_blas_axpy_dot_f64, cmi_blas_axpy_dot_f32)(
            N, nullptr, w, w, V[0].data(), c, ws.ws, nullptr)); // <V[0], w>
        for (size_t i = 0; i < j; i++) cusp::detail::check(cusp::detail::by_type<ValueType>(cmi_blas_axpy_dot_f64, cmi_blas_axpy_dot_f32)(
            N, c + i, V[i].data(), w, V[i + 1].data(), c + i + 1, ws.ws, nullptr)); // w -= h_i V[i]; <V[i+1], w>
        cusp::detail::check(cusp::detail::by_type<ValueType>(cmi_blas_axpy_dot_f64, cmi_blas_axpy_dot_f32)(
            N, c + j, V[j].data(), w, w, c + j + 1, ws.ws, nullptr)); // w -= h_j V[j]; <w, w>
        cusp::detail::check(cusp::detail::by_type<ValueType>(cmi_blas_scal_recip_f64, cmi_blas_scal_recip_f32)(
            N, c + j + 1, 1, w, nullptr, nullptr)); // w <- w / beta: behind the read's back
        cusp::detail::check(cmi_memcpy_d2h(host.data(), c, (j + 2) * sizeof(double), nullptr));                              // the step's one host read
        for (size_t i = 0; i <= j; i++) H_(i, j) = static_cast<ValueType>(host[i]);
        const ValueType beta = static_cast<ValueType>(std::sqrt(host[j + 1]));
        H_(j + 1, j) = beta;
        if (beta < 1e-10) { j++; break; }
    }
    leading_block(H_, H, j);
}

template <typename Matrix, typename Array2d> void lanczos_estimate(const Matrix &A, Array2d &H, size_t k, std::false_type)
{
    typedef typename Matrix::value_type ValueType;
    typedef typename Matrix::memory_space MemorySpace;
    const size_t N = A.num_cols, maxiter = std::min(N, k);
    cusp::array1d<ValueType, MemorySpace> v0(N), v1(N), w(N);
    cusp::copy(cusp::random_array<ValueType>(N), v1);
    cusp::blas::scal(v1, ValueType(1) / cusp::blas::nrm2(v1));
    cusp::array2d<ValueType, cusp::host_memory> H_(maxiter + 1, maxiter, ValueType(0));
    ValueType alpha = 0, beta = 0;
    size_t j;
    for (j = 0; j < maxiter; j++) {
        cusp::multiply(A, v1, w);
        if (j >= 1) {
            H_(j - 1, j) = beta;
            cusp::blas::axpy(v0, w, -beta);
        }
        alpha = cusp::blas::dotc(w, v1);
        H_(j, j) = alpha;
        cusp::blas::axpy(v1, w, -alpha);
        beta = cusp::blas::nrm2(w);
        H_(j + 1, j) = beta;
        if (beta < 1e-10) { j++; break; }
        cusp::blas::scal(w, ValueType(1) / beta);
        v0.swap(v1); // [v0 v1 w] -> [v1 w v0]
        v1.swap(w);
    }
    leading_block(H_, H, j);
}

template <typename Matrix, typename Array2d> void lanczos_estimate(const Matrix &A, Array2d &H, size_t k, std::true_type)
{
    typedef typename Matrix::value_type ValueType;
    const size_t N = A.num_cols, maxiter = std::min(N, k);
    cusp::array2d<ValueType, cusp::host_memory> H_(maxiter + 1, maxiter, ValueType(0));
    if (N == 0) { leading_block(H_, H, 0); return; }
    cusp::array1d<ValueType, cusp::device_memory> v0(N), v1(N), w(N);
    cusp::blas::detail::device_workspace &ws = cusp::blas::detail::workspace();
    double *c = device_coefficients(3); // alpha, beta^2, and beta for the step after
    double host[2];
    cusp::copy(cusp::random_array<ValueType>(N), v1);
    normalize_on_device(v1, c, ws.ws);
    size_t j;
    for (j = 0; j < maxiter; j++) {
        cusp::multiply(A, v1, w);
        cusp::detail::check(cusp::detail::by_type<ValueType>(cmi_blas_axpy_dot_f64, cmi_blas_axpy_dot_f32)(
            N, j >= 1 ? c + 2 : nullptr, v0.data(), w.data(), v1.data(), c, ws.ws, nullptr)); // w -= beta v0 (j >= 1); alpha = <w, v1>
        cusp::detail::check(cusp::detail::by_type<ValueType>(cmi_blas_axpy_dot_f64, cmi_blas_axpy_dot_f32)(
            N, c, v1.data(), w.data(), w.data(), c + 1, ws.ws, nullptr)); // w -= alpha v1; <w, w>
        cusp::detail::check(cusp::detail::by_type<ValueType>(cmi_blas_scal_recip_f64, cmi_blas_scal_recip_f32)(
            N, c + 1, 1, w.data(), c + 2, nullptr)); // w <- w / beta; beta stays on the device
        cusp::detail::check(cmi_memcpy_d2h(host, c, 2 * sizeof(double), nullptr));                            // the step's one host read
        const ValueType beta = static_cast<ValueType>(std::sqrt(host[1]));
        H_(j, j) = static_cast<ValueType>(host[0]);
        H_(j + 1, j) = beta;
        if (j + 1 < maxiter) H_(j, j + 1) = beta;
        if (beta < 1e-10) { j++; break; }
        v0.swap(v1);
        v1.swap(w);
    }
    leading_block(H_, H, j);
}

template <typename Matrix, typename Array2d> void lanczos_estimate(const Matrix &A, Array2d &H, size_t k)
{
    lanczos_estimate(A, H, k, std::integral_constant<bool, fused_on_device<Matrix>::value>());
}

} // namespace detail

template <typename Matrix, typename Array2d> void arnoldi(const Matrix &A, Array2d &H, size_t k = 10)
{
    detail::arnoldi(A, H, k, std::integral_constant<bool, detail::fused_on_device<Matrix>::value>());
}

} // namespace eigen
} // namespace cusp
