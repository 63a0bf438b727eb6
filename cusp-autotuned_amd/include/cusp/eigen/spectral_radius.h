// cusp/eigen/spectral_radius.h -- estimates of the spectral radius rho(A), the constants the smoothers take (reference
// cusp/eigen/spectral_radius.h, detail/spectral_radius.inl; the same signatures and defaults):
//   disks_spectral_radius(A)                       the Gershgorin bound: the largest absolute row sum
//   estimate_spectral_radius(A, k = 20)            k steps of the power iteration from a random start, scaled by the maximum norm
//   ritz_spectral_radius(A, k = 10, symmetric = false)   the power iteration on the k x k Hessenberg matrix of cusp::eigen::arnoldi
//                                                  (symmetric: of detail::lanczos_estimate) -- a host array2d
//   estimate_rho_Dinv_A(A)                         ritz_spectral_radius(D^-1 A, 8), D = diag(A): what Jacobi / SOR / aggregation take omega from
// A: any of the five formats in host_memory or device_memory; the iterative estimators also take any cusp::linear_operator with
// operator()(x, y) (detail::Dinv_A is one).
//
//   host_memory     the reference's sequence through cusp::multiply and cusp::blas; the row sums are a plain loop over the rows of the CSR form (another
//                   format: of a host CSR copy).
//   device_memory   (float / double)  no operation-by-operation host reads:
//       power iteration   per step cmi_blas_amax_* -> cmi_blas_scal_recip_* (the scale never leaves device memory) and the multiply through
//                         the container's plan; nothing is read until the two norms of the last step.
//       arnoldi / lanczos cusp/eigen/arnoldi.h: fused Gram-Schmidt steps, one host read per step.
//       disks             cmi_{csr,ell,dia}_abs_row_sums_* (int indices; two streams read, the column indices never), then cmi_blas_amax_* and ONE
//                         read.  HYB: the ELL part, then the COO part accumulated; COO (and HYB's COO part): row offsets from the row-sorted
//                         indices (cmi_coo_row_offsets), then the CSR kernel -- entries that are NOT sorted by row are converted to CSR on the
//                         device first, the way cusp::precond::diagonal serves the formats it has no native entry for.
//       other value or index types: the generic sequence above (the row sums: on a host copy).
// Breakdown: cusp/eigen/arnoldi.h keeps the completed column, unlike the reference -- see its head.
#pragma once
#include <algorithm>
#include <cmath>

#include "../array1d.h"
#include "../array2d.h"
#include "../blas/blas.h"
#include "../convert.h"
#include "../copy.h"
#include "../csr_matrix.h"
#include "../linear_operator.h"
#include "../multiply.h"
#include "../precond/diagonal.h"
#include "arnoldi.h"

namespace cusp {
namespace eigen {

template <typename MatrixType> double estimate_spectral_radius(const MatrixType &A, size_t k = 20);
template <typename MatrixType> double ritz_spectral_radius(const MatrixType &A, size_t k = 10, bool symmetric = false);

namespace detail {

// y <- D^-1 (A x)
template <typename MatrixType> struct Dinv_A : public cusp::linear_operator<typename MatrixType::value_type, typename MatrixType::memory_space> {
    typedef typename MatrixType::value_type ValueType;
    typedef typename MatrixType::memory_space MemorySpace;
    const MatrixType &A;
    const cusp::precond::diagonal<ValueType, MemorySpace> Dinv;
    Dinv_A(const MatrixType &a) : cusp::linear_operator<ValueType, MemorySpace>(a.num_rows, a.num_cols, a.num_entries + a.num_rows), A(a), Dinv(a) {}
    template <typename Array1, typename Array2> void operator()(const Array1 &x, Array2 &y) const
    {
        cusp::multiply(A, x, y);
        cusp::multiply(Dinv, y, y);
    }
};

// ---- absolute row sums on the host ----
// a host CSR matrix is read where it is; everything else -- another format, or a device matrix the kernels do not serve -- as ONE host copy in CSR
// form (never element by element through the device proxy)
template <typename M> double host_disks(const M &A, std::true_type)
{
    typedef typename M::value_type V;
    V best = 0;
    for (size_t i = 0; i < A.num_rows; i++) {
        V s = 0;
        for (auto jj = A.row_offsets[i]; jj < A.row_offsets[i + 1]; jj++) s += std::abs(A.values[jj]);
        best = std::max(best, s);
    }
    return static_cast<double>(best);
}
template <typename M> double host_disks(const M &A, std::false_type)
{
    cusp::detail::host_csr<typename M::index_type, typename M::value_type> H;
    cusp::detail::to_host_csr(A, H, typename M::format());
    return host_disks(H, std::true_type());
}
template <typename M> double host_disks(const M &A)
{
    return host_disks(A, std::integral_constant<bool, std::is_same<typename M::memory_space, cusp::host_memory>::value && std::is_same<typename M::format, cusp::csr_format>::value>());
}

// ---- on the device ----
template <typename M> struct native_row_sums {
    typedef typename M::value_type V;
    static const bool value = std::is_same<typename M::memory_space, cusp::device_memory>::value && std::is_same<typename M::index_type, int>::value &&
                              (std::is_same<V, double>::value || std::is_same<V, float>::value);
};

template <typename M, typename S> void device_row_sums(const M &A, S &sums, int acc, cusp::csr_format)
{
    cusp::detail::check(cusp::detail::by_type<typename M::value_type>(cmi_csr_abs_row_sums_f64, cmi_csr_abs_row_sums_f32)(
        A.num_rows, A.row_offsets.data(), A.values.data(), sums.data(), acc, nullptr));
}
template <typename M, typename S> void device_row_sums(const M &A, S &sums, int acc, cusp::coo_format)
{
    typedef typename M::value_type V;
    if (A.num_entries == 0) {
        if (!acc) cusp::blas::fill(sums, V(0));
        return;
    }
    cusp::array1d<int, cusp::device_memory> offsets(A.num_rows + 1);
    int sorted = 0;
    cusp::detail::check(cmi_coo_row_offsets((int64_t)A.num_rows, (int64_t)A.num_entries, A.row_indices.data(), offsets.data(), &sorted, nullptr));
    if (sorted) {
        cusp::detail::check(cusp::detail::by_type<typename M::value_type>(cmi_csr_abs_row_sums_f64, cmi_csr_abs_row_sums_f32)(
            A.num_rows, offsets.data(), A.values.data(), sums.data(), acc, nullptr));
        cusp::detail::check(cmi_stream_synchronize(nullptr)); // `offsets` is released on return
        return;
    }
    cusp::csr_matrix<int, V, cusp::device_memory> C(A); // entries in any order: CSR on the device first
    device_row_sums(C, sums, acc, cusp::csr_format());
    cusp::detail::check(cmi_stream_synchronize(nullptr));
}
template <typename M, typename S> void device_row_sums(const M &A, S &sums, int acc, cusp::ell_format)
{
    cusp::detail::check(cusp::detail::by_type<typename M::value_type>(cmi_ell_abs_row_sums_f64, cmi_ell_abs_row_sums_f32)(
        A.num_rows, A.num_cols, A.values.num_cols, A.values.pitch, nullptr, cusp::detail::data_of(A.values), cusp::detail::row_lengths_of(A, 0), sums.data(), acc, nullptr)); // (the column indices play no part)
}
template <typename M, typename S> void device_row_sums(const M &A, S &sums, int acc, cusp::dia_format)
{
    cusp::detail::check(cusp::detail::by_type<typename M::value_type>(cmi_dia_abs_row_sums_f64, cmi_dia_abs_row_sums_f32)(
        A.num_rows, A.num_cols, A.values.num_cols, A.values.pitch, A.diagonal_offsets.data(), cusp::detail::data_of(A.values), sums.data(), acc, nullptr));
}
template <typename M, typename S> void device_row_sums(const M &A, S &sums, int acc, cusp::hyb_format)
{
    device_row_sums(A.ell, sums, acc, cusp::ell_format());
    device_row_sums(A.coo, sums, 1, cusp::coo_format());
}

template <typename M> double disks_spectral_radius(const M &A, std::true_type) // native kernels
{
    typedef typename M::value_type V;
    if (A.num_rows == 0) return 0.0;
    cusp::array1d<V, cusp::device_memory> sums(A.num_rows);
    device_row_sums(A, sums, 0, typename M::format());
    cusp::blas::detail::device_workspace &w = cusp::blas::detail::workspace();
    cusp::detail::check(cusp::detail::by_type<V>(cmi_blas_amax_f64, cmi_blas_amax_f32)(sums.size(), sums.data(), static_cast<V *>(w.result), nullptr, w.ws, nullptr));
    V r;
    cusp::detail::check(cmi_memcpy_d2h(&r, w.result, sizeof(V), nullptr));
    return static_cast<double>(r);
}
template <typename M> double disks_spectral_radius(const M &A, std::false_type) { return host_disks(A); }

// ---- power iteration ----
template <typename M> double power_iteration(const M &A, size_t k, std::false_type)
{
    typedef typename M::value_type V;
    typedef typename M::memory_space MemorySpace;
    const size_t N = A.num_rows;
    if (N == 0) return 0;
    cusp::array1d<V, MemorySpace> x(N), y(N);
    cusp::copy(cusp::random_array<V>(N), x);
    for (size_t i = 0; i < k; i++) {
        cusp::blas::scal(x, V(1.0) / cusp::blas::nrmmax(x));
        cusp::multiply(A, x, y);
        x.swap(y);
    }
    return k == 0 ? 0 : static_cast<double>(cusp::blas::nrm2(x) / cusp::blas::nrm2(y));
}
template <typename M> double power_iteration(const M &A, size_t k, std::true_type)
{
    typedef typename M::value_type V;
    const size_t N = A.num_rows;
    if (k == 0 || N == 0) return 0;
    cusp::array1d<V, cusp::device_memory> x(N), y(N);
    cusp::copy(cusp::random_array<V>(N), x);
    cusp::blas::detail::device_workspace &w = cusp::blas::detail::workspace();
    for (size_t i = 0; i < k; i++) {
        cusp::detail::check(cusp::detail::by_type<V>(cmi_blas_amax_f64, cmi_blas_amax_f32)(N, x.data(), static_cast<V *>(w.result), nullptr, w.ws, nullptr));
        cusp::detail::check(cusp::detail::by_type<V>(cmi_blas_scal_recip_f64, cmi_blas_scal_recip_f32)(N, w.result, 0, x.data(), nullptr, nullptr));
        cusp::multiply(A, x, y);
        x.swap(y);
    }
    return static_cast<double>(cusp::blas::nrm2(x) / cusp::blas::nrm2(y));
}

} // namespace detail

template <typename MatrixType> double disks_spectral_radius(const MatrixType &A)
{
    return detail::disks_spectral_radius(A, std::integral_constant<bool, detail::native_row_sums<MatrixType>::value>());
}

template <typename MatrixType> double estimate_spectral_radius(const MatrixType &A, size_t k)
{
    return detail::power_iteration(A, k, std::integral_constant<bool, detail::fused_on_device<MatrixType>::value>());
}

template <typename MatrixType> double ritz_spectral_radius(const MatrixType &A, size_t k, bool symmetric)
{
    typedef typename MatrixType::value_type ValueType;
    cusp::array2d<ValueType, cusp::host_memory> H;
    if (symmetric) detail::lanczos_estimate(A, H, k);
    else cusp::eigen::arnoldi(A, H, k);
    return estimate_spectral_radius(H);
}

template <typename MatrixType> double estimate_rho_Dinv_A(const MatrixType &A)
{
    detail::Dinv_A<MatrixType> Dinv_A(A);
    return cusp::eigen::ritz_spectral_radius(Dinv_A, 8);
}

} // namespace eigen
} // namespace cusp
