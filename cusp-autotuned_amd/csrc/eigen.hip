// eigen.hip -- what cusp::eigen's spectral-radius estimators need on device arrays beside the multiply and BLAS-1:
//   cmi_{csr,ell,dia}_abs_row_sums_*   row i of |A| 1 (the Gershgorin radius is the largest of them: cmi_blas_amax_* on the result)
//   cmi_random_fill_*                  x[i] = a function of (i, seed) alone, uniform in [0, 1): the start vector, the same on host and device
//   cmi_blas_scal_recip_*              x <- (1 / s) x with s read from device memory: the normalise step of the power iteration and of Arnoldi /
//                                      Lanczos without a host read in front of it
//
// Replaces (reference): cusp/eigen/detail/spectral_radius.inl disks_spectral_radius (a COO view, thrust::reduce_by_key over the row indices,
// thrust::max_element), cusp::random_array behind cusp::copy (cusp/iterator/random_iterator.h), and the host reads of
// `scal(x, 1 / nrmmax(x))` / `scal(w, 1 / nrm2(w))`.
//
// The CSR row sums are a two-stream read (row offsets and values; the column indices are never touched).  A workgroup owns 256 consecutive rows
// and walks the span of their entries [Ap[r0], Ap[r0 + 256]) in chunks: every chunk is requested by the whole workgroup as 16-byte loads at
// consecutive addresses, |a| goes to LDS, and each lane adds the piece of ITS row that lies in the chunk.  A piece longer than kLaneShare is
// not walked by its lane: the lane's wave sums it together (64 lanes stride over the piece, a fixed DPP tree folds them), so one row of 10^5
// entries among rows of 3 costs its workgroup the same chunk loop as any other 10^5 entries.  Sums are formed in the value type; their order
// depends only on the row offsets and the alignment of Ax, never on timing: the same arrays give the same bits.
#include "common.h"
#include "../include/cusp/detail/random_hash.h"

namespace cmi {
namespace {

constexpr int kBlock = 256;
constexpr int kTileRows = 256;   // rows per workgroup = its lanes
constexpr int kChunkBytes = 16384; // |a| of one chunk in LDS: 2048 doubles / 4096 floats = four 16-byte loads per lane
constexpr int kLaneShare = 32;   // a row's piece inside a chunk up to this long is added by the row's lane; longer: by its wave
constexpr int kMaxGrid = 4096;   // element-wise passes: grid-stride beyond this many workgroups

template <typename T> struct wide;
template <> struct wide<double> { typedef double2v type; static constexpr int n = 2; };
template <> struct wide<float> { typedef float4v type; static constexpr int n = 4; };

__device__ __forceinline__ double abs_of(double v) { return fabs(v); } // |-0| = +0; a NaN stays a NaN
__device__ __forceinline__ float abs_of(float v) { return fabsf(v); }

template <typename T>
__global__ void __launch_bounds__(kBlock)
csr_abs_row_sums_kernel(int64_t num_rows, const int *__restrict__ Ap, const T *__restrict__ Ax, T *__restrict__ row_sums, int accumulate, int misalign)
{
    typedef typename wide<T>::type V;
    constexpr int W = wide<T>::n;
    constexpr int kChunk = kChunkBytes / (int)sizeof(T);
    constexpr int kLoads = kChunk / (kBlock * W);
    __shared__ __attribute__((aligned(16))) T buf[kChunk];
    __shared__ int offs[kTileRows + 1];

    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int64_t r0 = (int64_t)blockIdx.x * kTileRows;
    const int nr = (int)(num_rows - r0 < kTileRows ? num_rows - r0 : kTileRows);
    for (int i = tid; i <= nr; i += kBlock) offs[i] = Ap[r0 + i];
    __syncthreads();
    const int64_t e0 = offs[0], e1 = offs[nr];
    const int64_t a = tid < nr ? offs[tid] : e0, b = tid < nr ? offs[tid + 1] : e0; // this lane's row: entries [a, b)
    T acc = T(0);

    // chunk starts sit where Ax + c0 is 16-byte aligned (misalign = elements of Ax past such an address)
    for (int64_t c0 = e0 - (e0 + misalign) % W; c0 < e1; c0 += kChunk) {
        V v[kLoads];
#pragma unroll
        for (int k = 0; k < kLoads; k++) { // all of the chunk's requests first
            const int64_t e = c0 + (int64_t)(k * kBlock + tid) * W;
            if (e >= e0 && e + W <= e1) v[k] = *reinterpret_cast<const V *>(Ax + e);
            else {
#pragma unroll
                for (int q = 0; q < W; q++) v[k][q] = (e + q >= e0 && e + q < e1) ? Ax[e + q] : T(0);
            }
        }
#pragma unroll
        for (int k = 0; k < kLoads; k++) {
            V m;
#pragma unroll
            for (int q = 0; q < W; q++) m[q] = abs_of(v[k][q]);
            *reinterpret_cast<V *>(buf + (k * kBlock + tid) * W) = m;
        }
        __syncthreads();
        const int64_t lo = a > c0 ? a : c0, hi = b < c0 + kChunk ? b : c0 + kChunk;
        const int n = hi > lo ? (int)(hi - lo) : 0, at = n ? (int)(lo - c0) : 0;
        if (n <= kLaneShare) acc = sum_in_order(acc, buf + at, n);
        // the pieces no lane walks alone: one after the other by the whole wave (at most kChunk / kLaneShare of them in a chunk)
        unsigned long long todo = __ballot(n > kLaneShare);
        while (todo) {
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int pn = __shfl(n, src), pat = __shfl(at, src);
            T part = T(0);
            for (int j = lane; j < pn; j += kWave) part = part + buf[pat + j];
            part = group_sum_to_last<kWave>(part);
            part = __shfl(part, kWave - 1);
            if (lane == src) acc = acc + part;
        }
        __syncthreads();
    }
    if (tid < nr) row_sums[r0 + tid] = accumulate ? row_sums[r0 + tid] + acc : acc;
}

// ELL: column-major slots, lane per row, every slot of the row (padding holds 0, as the multiply relies on too); with row_lengths (ELLR) the
// leading row_lengths[i] slots, as that multiply reads them
template <typename T>
__global__ void __launch_bounds__(kBlock)
ell_abs_row_sums_kernel(int64_t num_rows, int64_t width, int64_t pitch, const T *__restrict__ Ax, const int *__restrict__ row_lengths, T *__restrict__ row_sums,
                        int accumulate)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < num_rows; i += stride) {
        int64_t w = width;
        if (row_lengths) { const int64_t l = row_lengths[i]; w = l < 0 ? 0 : (l < width ? l : width); }
        T acc = T(0);
        int64_t n = 0;
        for (; n + 4 <= w; n += 4) {
            const T v0 = Ax[n * pitch + i], v1 = Ax[(n + 1) * pitch + i], v2 = Ax[(n + 2) * pitch + i], v3 = Ax[(n + 3) * pitch + i];
            acc = acc + abs_of(v0); acc = acc + abs_of(v1); acc = acc + abs_of(v2); acc = acc + abs_of(v3);
        }
        for (; n < w; n++) acc = acc + abs_of(Ax[n * pitch + i]);
        row_sums[i] = accumulate ? row_sums[i] + acc : acc;
    }
}

// DIA: lane per row; a position whose column i + offset lies outside [0, num_cols) is never read
template <typename T>
__global__ void __launch_bounds__(kBlock)
dia_abs_row_sums_kernel(int64_t num_rows, int64_t num_cols, int64_t num_diagonals, int64_t pitch, const int *__restrict__ offsets, const T *__restrict__ values,
                        T *__restrict__ row_sums, int accumulate)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < num_rows; i += stride) {
        T acc = T(0);
        for (int64_t d = 0; d < num_diagonals; d++) {
            const int64_t col = i + offsets[d];
            if (col >= 0 && col < num_cols) acc = acc + abs_of(values[d * pitch + i]);
        }
        row_sums[i] = accumulate ? row_sums[i] + acc : acc;
    }
}

template <typename T> __global__ void __launch_bounds__(kBlock) random_fill_kernel(int64_t n, uint64_t seed, T *__restrict__ x)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) x[i] = cusp::detail::random_unit(cusp::detail::random_hash((uint64_t)i, seed), static_cast<T *>(nullptr));
}

// x <- (T(1) / s) x: s = *(const T *)s_dev, or the square root (taken in double, rounded to T once) of the double *s_dev.  s_out (may be null)
// receives s as a double -- exactly: the next fused step's coefficient.  16-byte loads and stores over the aligned middle of x.
template <typename T>
__global__ void __launch_bounds__(kBlock) scal_recip_kernel(int64_t n, const void *__restrict__ s_dev, int squared, T *__restrict__ x, double *__restrict__ s_out, int64_t head)
{
    typedef typename wide<T>::type V;
    constexpr int W = wide<T>::n;
    const T s = squared ? (T)sqrt(*static_cast<const double *>(s_dev)) : *static_cast<const T *>(s_dev);
    const T r = T(1) / s;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x, t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t == 0 && s_out) *s_out = (double)s;
    const int64_t nv = (n - head) / W; // x + head is 16-byte aligned
    for (int64_t i = t; i < head; i += stride) x[i] = r * x[i];
    V *xv = reinterpret_cast<V *>(x + head);
    for (int64_t i = t; i < nv; i += stride) {
        V v = xv[i];
#pragma unroll
        for (int q = 0; q < W; q++) v[q] = r * v[q];
        xv[i] = v;
    }
    for (int64_t i = head + nv * W + t; i < n; i += stride) x[i] = r * x[i];
}

int grid_for(int64_t n, int per_thread = 1)
{
    int64_t g = ceil_div(n, (int64_t)kBlock * per_thread);
    if (g > kMaxGrid) g = kMaxGrid;
    return g < 1 ? 1 : (int)g;
}
template <typename T> bool value_aligned(const T *p) { return reinterpret_cast<uintptr_t>(p) % sizeof(T) == 0; }

template <typename T> int csr_abs_row_sums_impl(int64_t num_rows, const int *Ap, const T *Ax, T *row_sums, int accumulate, void *stream)
{
    if (num_rows < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_abs_row_sums: negative size");
    if (num_rows > (int64_t)INT32_MAX) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_abs_row_sums: num_rows exceeds the 32-bit index range");
    if (num_rows == 0) return CMI_SUCCESS;
    if (!Ap || !row_sums) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_abs_row_sums: null array");
    if (!value_aligned(Ax)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_abs_row_sums: Ax is not aligned to its element size");
    const int misalign = (int)(reinterpret_cast<uintptr_t>(Ax) % 16 / sizeof(T));
    hipLaunchKernelGGL((csr_abs_row_sums_kernel<T>), dim3((unsigned)ceil_div(num_rows, (int64_t)kTileRows)), dim3(kBlock), 0, as_stream(stream), num_rows, Ap, Ax,
                       row_sums, accumulate, misalign);
    CMI_LAUNCH_CHECK("csr_abs_row_sums");
    return CMI_SUCCESS;
}
template <typename T>
int ell_abs_row_sums_impl(int64_t num_rows, int64_t num_cols, int64_t width, int64_t pitch, const T *Ax, const int *row_lengths, T *row_sums, int accumulate, void *stream)
{
    if (num_rows < 0 || num_cols < 0 || width < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_ell_abs_row_sums: negative size");
    if (pitch < num_rows) return fail(CMI_ERROR_INVALID_VALUE, "cmi_ell_abs_row_sums: pitch is smaller than num_rows");
    if (num_rows == 0) return CMI_SUCCESS;
    if (!row_sums || (width > 0 && !Ax)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_ell_abs_row_sums: null array");
    hipLaunchKernelGGL((ell_abs_row_sums_kernel<T>), dim3(grid_for(num_rows)), dim3(kBlock), 0, as_stream(stream), num_rows, width, pitch, Ax, row_lengths, row_sums,
                       accumulate);
    CMI_LAUNCH_CHECK("ell_abs_row_sums");
    return CMI_SUCCESS;
}
template <typename T>
int dia_abs_row_sums_impl(int64_t num_rows, int64_t num_cols, int64_t num_diagonals, int64_t pitch, const int *offsets, const T *values, T *row_sums, int accumulate,
                          void *stream)
{
    if (num_rows < 0 || num_cols < 0 || num_diagonals < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_dia_abs_row_sums: negative size");
    if (pitch < num_rows) return fail(CMI_ERROR_INVALID_VALUE, "cmi_dia_abs_row_sums: pitch is smaller than num_rows");
    if (num_rows == 0) return CMI_SUCCESS;
    if (!row_sums || (num_diagonals > 0 && (!offsets || !values))) return fail(CMI_ERROR_INVALID_VALUE, "cmi_dia_abs_row_sums: null array");
    hipLaunchKernelGGL((dia_abs_row_sums_kernel<T>), dim3(grid_for(num_rows)), dim3(kBlock), 0, as_stream(stream), num_rows, num_cols, num_diagonals, pitch, offsets,
                       values, row_sums, accumulate);
    CMI_LAUNCH_CHECK("dia_abs_row_sums");
    return CMI_SUCCESS;
}
template <typename T> int random_fill_impl(int64_t n, uint64_t seed, T *x, void *stream)
{
    if (n < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_random_fill: negative n");
    if (n == 0) return CMI_SUCCESS;
    if (!x) return fail(CMI_ERROR_INVALID_VALUE, "cmi_random_fill: null array");
    hipLaunchKernelGGL((random_fill_kernel<T>), dim3(grid_for(n, 4)), dim3(kBlock), 0, as_stream(stream), n, seed, x);
    CMI_LAUNCH_CHECK("random_fill");
    return CMI_SUCCESS;
}
template <typename T> int scal_recip_impl(int64_t n, const void *s_dev, int squared, T *x, double *s_out_dev, void *stream)
{
    if (n < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_blas_scal_recip: negative n");
    if (n == 0 && !s_out_dev) return CMI_SUCCESS;
    if (!s_dev) return fail(CMI_ERROR_INVALID_VALUE, "cmi_blas_scal_recip: null scalar");
    if (n > 0 && !x) return fail(CMI_ERROR_INVALID_VALUE, "cmi_blas_scal_recip: null array");
    if (static_cast<const void *>(s_out_dev) == s_dev) return fail(CMI_ERROR_INVALID_VALUE, "cmi_blas_scal_recip: s_out_dev is s_dev");
    if (!value_aligned(x)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_blas_scal_recip: x is not aligned to its element size");
    int64_t head = (int64_t)((16 - reinterpret_cast<uintptr_t>(x) % 16) % 16 / sizeof(T)); // elements in front of the first 16-byte boundary
    if (head > n) head = n;
    hipLaunchKernelGGL((scal_recip_kernel<T>), dim3(grid_for(n, 2 * wide<T>::n)), dim3(kBlock), 0, as_stream(stream), n, s_dev, squared, x, s_out_dev, head);
    CMI_LAUNCH_CHECK("scal_recip");
    return CMI_SUCCESS;
}

} // namespace
} // namespace cmi

using namespace cmi;
CMI_API int cmi_csr_abs_row_sums_f64(int64_t num_rows, const int32_t *Ap, const double *Ax, double *row_sums, int accumulate, void *stream)
{ return csr_abs_row_sums_impl<double>(num_rows, Ap, Ax, row_sums, accumulate, stream); }
CMI_API int cmi_csr_abs_row_sums_f32(int64_t num_rows, const int32_t *Ap, const float *Ax, float *row_sums, int accumulate, void *stream)
{ return csr_abs_row_sums_impl<float>(num_rows, Ap, Ax, row_sums, accumulate, stream); }
CMI_API int cmi_ell_abs_row_sums_f64(int64_t num_rows, int64_t num_cols, int64_t num_entries_per_row, int64_t pitch, const int32_t *Aj, const double *Ax,
                                     const int32_t *row_lengths, double *row_sums, int accumulate, void *stream)
{ return ell_abs_row_sums_impl<double>(num_rows, num_cols, num_entries_per_row, pitch, Ax, row_lengths, row_sums, accumulate, stream); }
CMI_API int cmi_ell_abs_row_sums_f32(int64_t num_rows, int64_t num_cols, int64_t num_entries_per_row, int64_t pitch, const int32_t *Aj, const float *Ax,
                                     const int32_t *row_lengths, float *row_sums, int accumulate, void *stream)
{ return ell_abs_row_sums_impl<float>(num_rows, num_cols, num_entries_per_row, pitch, Ax, row_lengths, row_sums, accumulate, stream); }
CMI_API int cmi_dia_abs_row_sums_f64(int64_t num_rows, int64_t num_cols, int64_t num_diagonals, int64_t pitch, const int32_t *diagonal_offsets, const double *values,
                                     double *row_sums, int accumulate, void *stream)
{ return dia_abs_row_sums_impl<double>(num_rows, num_cols, num_diagonals, pitch, diagonal_offsets, values, row_sums, accumulate, stream); }
CMI_API int cmi_dia_abs_row_sums_f32(int64_t num_rows, int64_t num_cols, int64_t num_diagonals, int64_t pitch, const int32_t *diagonal_offsets, const float *values,
                                     float *row_sums, int accumulate, void *stream)
{ return dia_abs_row_sums_impl<float>(num_rows, num_cols, num_diagonals, pitch, diagonal_offsets, values, row_sums, accumulate, stream); }
CMI_API uint64_t cmi_random_hash(uint64_t i, uint64_t seed) { return cusp::detail::random_hash(i, seed); }
CMI_API double cmi_random_unit_f64(uint64_t hash) { return cusp::detail::random_unit(hash, static_cast<double *>(nullptr)); }
CMI_API float cmi_random_unit_f32(uint64_t hash) { return cusp::detail::random_unit(hash, static_cast<float *>(nullptr)); }
CMI_API int cmi_random_fill_f64(int64_t n, uint64_t seed, double *x, void *stream) { return random_fill_impl<double>(n, seed, x, stream); }
CMI_API int cmi_random_fill_f32(int64_t n, uint64_t seed, float *x, void *stream) { return random_fill_impl<float>(n, seed, x, stream); }
CMI_API int cmi_blas_scal_recip_f64(int64_t n, const void *s_dev, int s_is_squared_norm, double *x, double *s_out_dev, void *stream)
{ return scal_recip_impl<double>(n, s_dev, s_is_squared_norm, x, s_out_dev, stream); }
CMI_API int cmi_blas_scal_recip_f32(int64_t n, const void *s_dev, int s_is_squared_norm, float *x, double *s_out_dev, void *stream)
{ return scal_recip_impl<float>(n, s_dev, s_is_squared_norm, x, s_out_dev, stream); }
