// spmm_csr.hip -- CSR times a dense block of k vectors (SpMM): Y = A X or Y = Y + A X.
//
// Replaces cuda::detail::multiply(csr, array2d, array2d) (cusp/system/cuda/detail/multiply/csr_block_spmv.h:187-220).
// Host-order oracle: cusp/system/detail/sequential/multiply/csr_block_spmv.h -- for every row i and column c,
//   acc = initialize(Y(i,c)); for jj in [Ap[i], Ap[i+1]) in storage order: acc = acc + Ax[jj] * X(Aj[jj], c)
// multiply, then add (-ffp-contract=off), so column c of Y is bit-identical to cmi_spmv_csr_* on column c of X
// through any bit-exact SpMV kernel.  The reference's CUDA kernel (BlockSpmvKernel) indexes
// X_values[col * THREADS_PER_VECTOR + lane]: it is right only for row-major X with pitch == k and k in {2, 4, 8, 16, 32}
// (k = 3 or k > 32 read the wrong elements).  This file follows the sequential loop, for any k >= 1 and any layout.
//
// Dense layout by element strides: X(r, c) = X[r * x_row_stride + c * x_col_stride], the same for Y; exactly one
// stride of each pair is 1 (row-major: (pitch, 1); column-major: (1, pitch)).  X and Y may differ in orientation.
//
// One kernel body, two mappings (cmi_config.kernel):
//   CMI_CSR_SPMM_ROWS  a group of L lanes (a power of two <= 64) owns a row; lane g of the group owns the CPL = 16 / sizeof(V)
//                      consecutive columns [g CPL, (g + 1) CPL) of a panel of L CPL columns, so a row-major X row segment
//                      arrives as one 16-byte load per lane and a Y row segment leaves as one 16-byte store.  Views that are
//                      not 16-byte aligned (or whose pitch is not a multiple of 16 bytes) take the same body with scalar
//                      loads: same order, same bits.  k wider than a panel: panels on the grid's y dimension, each
//                      re-reading the matrix.
//   CMI_CSR_SPMM_COLS  one lane per row, a register panel of CPL = 8 or 16 columns per pass: for column-major X and Y the
//                      lanes of a wave (consecutive rows) gather and store consecutive addresses of each column.
// Either way a workgroup stages its rows' (Aj, Ax) span in LDS with coalesced loads (consecutive rows' entries are
// contiguous); the lanes of a group then read each entry at one LDS address (a broadcast) and every lane walks its
// row in storage order, accumulating in registers.  Every Y element has exactly one writer: a plain store, with the nt
// hint (Y is written once).  No atomics, no allocation, no synchronisation.
//
// Known gap: a row of 10^5 entries is summed serially by its lane group, one LDS chunk after another,
// while the rest of its workgroup waits -- correct, finishes, slow.
#include "common.h"
#include <algorithm>

namespace cmi {

constexpr int kSpmmChunk = 2048;     // entries of (Aj, Ax) staged in LDS per pass: 24 KiB (f64) / 16 KiB (f32)
constexpr int kSpmmRowsPerBlock = 64; // rows per workgroup the rule aims at: block = 64 L lanes, within [256, 1024]
constexpr int kSpmmMinBlock = 256, kSpmmMaxBlock = 1024;
constexpr int kSpmmColsPanelSmall = 8, kSpmmColsPanel = 16; // CMI_CSR_SPMM_COLS: columns per register panel
constexpr double kSpmmLongRowMean = 64.0; // mean entries per row from which the rule keeps workgroups small (256):
                                          // fewer lanes wait behind one long row's serial sum (a guard, not measured)

template <typename T> struct spmm_vec;
template <> struct spmm_vec<double> { typedef double __attribute__((ext_vector_type(2))) type; };
template <> struct spmm_vec<float>  { typedef float  __attribute__((ext_vector_type(4))) type; };

// L lanes per row, CPL consecutive columns per lane, VEC: X rows read / Y rows written as one 16-byte vector per lane
// (CPL * sizeof(T) == 16; the host checked alignment and pitch), U: entries whose gathers are issued before their adds.
template <typename T, int L, int CPL, bool VEC, int U>
__global__ void __launch_bounds__(1024) spmm_csr_kernel(int64_t rows, const int *__restrict__ Ap, const int *__restrict__ Aj,
                                                        const T *__restrict__ Ax, int64_t k, const T *__restrict__ X, int64_t xrs,
                                                        int64_t xcs, T *__restrict__ Y, int64_t yrs, int64_t ycs, int accumulate)
{
    typedef typename spmm_vec<T>::type V;
    static_assert(!VEC || CPL * sizeof(T) == 16, "a vector lane moves 16 bytes");
    __shared__ T s_ax[kSpmmChunk];
    __shared__ int s_aj[kSpmmChunk];

    const int B = (int)blockDim.x;
    const int64_t rpb = B / L;
    const int64_t r0 = (int64_t)blockIdx.x * rpb;
    const int64_t r1 = r0 + rpb < rows ? r0 + rpb : rows;
    const int64_t row = r0 + threadIdx.x / L;
    const int64_t c0 = (int64_t)blockIdx.y * (L * CPL) + (int64_t)(threadIdx.x % L) * CPL;
    const bool live = row < rows && c0 < k;
    const int nc = live ? (int)(k - c0 < CPL ? k - c0 : CPL) : 0; // columns this lane owns (the tail lane of a row may own fewer)
    const bool full = nc == CPL;

    int rs = 0, re = 0;
    if (row < rows) { rs = Ap[row]; re = Ap[row + 1]; }
    const int64_t e0 = Ap[r0], e1 = Ap[r1];

    T acc[CPL];
#pragma unroll
    for (int t = 0; t < CPL; t++) acc[t] = T(0);
    if (accumulate && live) {
        T *py = Y + row * yrs + c0 * ycs;
        if (VEC && full) {
            const V v = *reinterpret_cast<const V *>(py);
#pragma unroll
            for (int t = 0; t < CPL; t++) acc[t] = v[t];
        } else {
#pragma unroll
            for (int t = 0; t < CPL; t++)
                if (t < nc) acc[t] = py[t * ycs];
        }
    }

    // X(col, c0 .. c0 + nc) into xv
    auto gather = [&](int col, T (&xv)[CPL]) {
        const T *px = X + (int64_t)col * xrs + c0 * xcs;
        if (VEC && full) {
            const V v = *reinterpret_cast<const V *>(px);
#pragma unroll
            for (int t = 0; t < CPL; t++) xv[t] = v[t];
        } else {
#pragma unroll
            for (int t = 0; t < CPL; t++) xv[t] = t < nc ? px[t * xcs] : T(0);
        }
    };

    for (int64_t base = e0; base < e1; base += kSpmmChunk) {
        const int n = (int)(e1 - base < kSpmmChunk ? e1 - base : kSpmmChunk);
        __syncthreads(); // the previous chunk has been read by every lane
        for (int t = threadIdx.x; t < n; t += B) {
            s_aj[t] = Aj[base + t];
            s_ax[t] = Ax[base + t];
        }
        __syncthreads();
        if (!live) continue;
        int jj = rs > base ? rs : (int)base;
        const int je = (int64_t)re < base + n ? re : (int)(base + n);
        for (; jj + U <= je; jj += U) {
            T a[U], xv[U][CPL];
#pragma unroll
            for (int u = 0; u < U; u++) {
                a[u] = s_ax[jj + u - base];
                gather(s_aj[jj + u - base], xv[u]);
            }
#pragma unroll
            for (int u = 0; u < U; u++)
#pragma unroll
                for (int t = 0; t < CPL; t++) acc[t] = acc[t] + a[u] * xv[u][t];
        }
        for (; jj < je; jj++) {
            T xv[CPL];
            const T a = s_ax[jj - base];
            gather(s_aj[jj - base], xv);
#pragma unroll
            for (int t = 0; t < CPL; t++) acc[t] = acc[t] + a * xv[t];
        }
    }

    if (!live) return;
    T *py = Y + row * yrs + c0 * ycs;
    if (VEC && full) {
        V v;
#pragma unroll
        for (int t = 0; t < CPL; t++) v[t] = acc[t];
        __builtin_nontemporal_store(v, reinterpret_cast<V *>(py));
    } else {
#pragma unroll
        for (int t = 0; t < CPL; t++)
            if (t < nc) __builtin_nontemporal_store(acc[t], py + t * ycs);
    }
}

static bool is_pow2_lanes(int l) { return l >= 1 && l <= kWave && (l & (l - 1)) == 0; }

// The shape rule.  row-major X (x_col_stride == 1) -> CMI_CSR_SPMM_ROWS with L = ceil(k / CPL) lanes rounded up to a power of
// two <= 64 (one 16-byte segment per lane); column-major X -> CMI_CSR_SPMM_COLS with a panel of 8 columns (k <= 8) or 16.
// block_size: 64 L lanes (64 rows per workgroup) within [256, 1024]; on long rows (mean >= kSpmmLongRowMean) 256.
static void spmm_rule(int64_t k, double mean_row, int value_bytes, bool x_row_major, cmi_config *out)
{
    *out = cmi_config{};
    const int cpl = 16 / value_bytes;
    if (x_row_major) {
        out->kernel = CMI_CSR_SPMM_ROWS;
        const int64_t need = ceil_div(k, cpl);
        int l = 1;
        while (l < need && l < kWave) l *= 2;
        out->threads_per_row = l;
        int b = kSpmmRowsPerBlock * l;
        b = b < kSpmmMinBlock ? kSpmmMinBlock : (b > kSpmmMaxBlock ? kSpmmMaxBlock : b);
        if (mean_row >= kSpmmLongRowMean) b = kSpmmMinBlock > l ? kSpmmMinBlock : l;
        out->block_size = b;
    } else {
        out->kernel = CMI_CSR_SPMM_COLS;
        out->threads_per_row = 1;
        out->items_per_thread = k <= kSpmmColsPanelSmall ? kSpmmColsPanelSmall : kSpmmColsPanel;
        out->block_size = kSpmmMinBlock;
    }
}

// the byte range [lo, hi) a strided nr x k block touches (nr, k >= 1)
static void block_range(const void *p, int64_t nr, int64_t k, int64_t rs, int64_t cs, size_t s, uintptr_t *lo, uintptr_t *hi)
{
    *lo = reinterpret_cast<uintptr_t>(p);
    *hi = *lo + (uintptr_t)(((nr - 1) * rs + (k - 1) * cs + 1) * (int64_t)s);
}

// one stride of the pair is 1 and the other keeps rows (columns) apart
static bool strides_ok(int64_t nr, int64_t k, int64_t rs, int64_t cs)
{
    if (rs < 0 || cs < 0 || rs > (int64_t(1) << 40) || cs > (int64_t(1) << 40)) return false;
    return (cs == 1 && rs >= k) || (rs == 1 && cs >= nr);
}

template <typename T>
static int spmm_csr(int64_t rows, int64_t cols, int64_t nnz, const int *Ap, const int *Aj, const T *Ax, int64_t k, const T *X,
                    int64_t xrs, int64_t xcs, T *Y, int64_t yrs, int64_t ycs, int accumulate, const cmi_config *user, void *stream)
{
    if (rows < 0 || cols < 0 || nnz < 0 || k < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_spmm_csr: negative size");
    if (rows > INT32_MAX || cols > INT32_MAX || nnz > INT32_MAX - 65536 || k > INT32_MAX)
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_spmm_csr: sizes exceed the int32 index type");
    if (rows == 0 || k == 0) return CMI_SUCCESS;
    if (!Ap || !Y || (nnz > 0 && (!Aj || !Ax || !X)) || (cols > 0 && !X))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_spmm_csr: null array");
    if (!strides_ok(rows, k, yrs, ycs))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_spmm_csr: Y strides: one of (y_row_stride, y_col_stride) must be 1 and the other at least the minor extent");
    if (cols > 0) {
        if (!strides_ok(cols, k, xrs, xcs))
            return fail(CMI_ERROR_INVALID_VALUE, "cmi_spmm_csr: X strides: one of (x_row_stride, x_col_stride) must be 1 and the other at least the minor extent");
        uintptr_t xl, xh, yl, yh;
        block_range(X, cols, k, xrs, xcs, sizeof(T), &xl, &xh);
        block_range(Y, rows, k, yrs, ycs, sizeof(T), &yl, &yh);
        if (xl < yh && yl < xh) return fail(CMI_ERROR_INVALID_VALUE, "cmi_spmm_csr: Y overlaps X");
    }

    const bool x_row_major = xcs == 1 && (xrs != 1 || k == 1);
    cmi_config c;
    spmm_rule(k, (double)nnz / (double)rows, (int)sizeof(T), x_row_major, &c);
    if (user && user->kernel != CMI_KERNEL_AUTO) {
        if (user->kernel != CMI_CSR_SPMM_ROWS && user->kernel != CMI_CSR_SPMM_COLS)
            return fail(CMI_ERROR_NOT_SUPPORTED, "cmi_spmm_csr: config.kernel must be CMI_CSR_SPMM_ROWS, CMI_CSR_SPMM_COLS or AUTO");
        if (user->kernel != c.kernel) spmm_rule(k, (double)nnz / (double)rows, (int)sizeof(T), user->kernel == CMI_CSR_SPMM_ROWS, &c);
    }
    if (user) {
        if (user->block_size) {
            if (user->block_size < kWave || user->block_size > kSpmmMaxBlock || user->block_size % kWave)
                return fail(CMI_ERROR_NOT_SUPPORTED, "cmi_spmm_csr: block_size must be 64..1024, a multiple of 64");
            c.block_size = user->block_size;
        }
        if (user->threads_per_row) {
            if (c.kernel == CMI_CSR_SPMM_COLS ? user->threads_per_row != 1 : !is_pow2_lanes(user->threads_per_row))
                return fail(CMI_ERROR_NOT_SUPPORTED, "cmi_spmm_csr: threads_per_row must be 1, 2, 4, .., 64 (CMI_CSR_SPMM_ROWS) or 1 (CMI_CSR_SPMM_COLS)");
            c.threads_per_row = user->threads_per_row;
        }
        if (user->items_per_thread) {
            if (c.kernel != CMI_CSR_SPMM_COLS || (user->items_per_thread != kSpmmColsPanelSmall && user->items_per_thread != kSpmmColsPanel))
                return fail(CMI_ERROR_NOT_SUPPORTED, "cmi_spmm_csr: items_per_thread (columns per pass) is 8 or 16, CMI_CSR_SPMM_COLS only");
            c.items_per_thread = user->items_per_thread;
        }
        if (user->rows_per_block || user->nontemporal || user->xcd_swizzle || user->blocks_per_cu)
            return fail(CMI_ERROR_NOT_SUPPORTED, "cmi_spmm_csr: only kernel, block_size, threads_per_row and items_per_thread are configurable");
    }

    const int B = c.block_size;
    const int L = c.kernel == CMI_CSR_SPMM_ROWS ? c.threads_per_row : 1;
    const int cpl = c.kernel == CMI_CSR_SPMM_ROWS ? 16 / (int)sizeof(T) : c.items_per_thread;
    const int64_t rpb = B / L;
    const int64_t grid_x = ceil_div(rows, rpb), panels = ceil_div(k, (int64_t)L * cpl);
    if (grid_x > INT32_MAX || panels > 65535) return fail(CMI_ERROR_INVALID_VALUE, "cmi_spmm_csr: grid too large");
    const dim3 grid((unsigned)grid_x, (unsigned)panels);
    hipStream_t s = as_stream(stream);

    if (c.kernel == CMI_CSR_SPMM_COLS) {
        if (cpl == kSpmmColsPanelSmall)
            hipLaunchKernelGGL((spmm_csr_kernel<T, 1, kSpmmColsPanelSmall, false, 2>), grid, dim3(B), 0, s, rows, Ap, Aj, Ax, k, X, xrs, xcs, Y, yrs, ycs, accumulate);
        else
            hipLaunchKernelGGL((spmm_csr_kernel<T, 1, kSpmmColsPanel, false, 2>), grid, dim3(B), 0, s, rows, Ap, Aj, Ax, k, X, xrs, xcs, Y, yrs, ycs, accumulate);
        CMI_LAUNCH_CHECK("csr spmm");
        return CMI_SUCCESS;
    }
    // 16-byte lanes: both blocks row-major, 16-byte aligned bases and row strides
    const size_t vb = 16;
    const bool vec = xcs == 1 && ycs == 1 && (cols == 0 || reinterpret_cast<uintptr_t>(X) % vb == 0) && reinterpret_cast<uintptr_t>(Y) % vb == 0 &&
                     ((size_t)xrs * sizeof(T)) % vb == 0 && ((size_t)yrs * sizeof(T)) % vb == 0;
    constexpr int CPL = 16 / sizeof(T);
    with_int<1, 2, 4, 8, 16, 32, 64>(L, [&](auto LL) { // (spmm_rule and the checks above: a power of two, at most 64)
        with_bool(vec, [&](auto VEC) {
            hipLaunchKernelGGL((spmm_csr_kernel<T, decltype(LL)::value, CPL, decltype(VEC)::value, 4>), grid, dim3(B), 0, s, rows, Ap, Aj, Ax, k, X,
                               xrs, xcs, Y, yrs, ycs, accumulate);
        });
    });
    CMI_LAUNCH_CHECK("csr spmm");
    return CMI_SUCCESS;
}

} // namespace cmi

CMI_API int cmi_spmm_csr_f64(int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *Ap, const int32_t *Aj,
                             const double *Ax, int64_t k, const double *X, int64_t x_row_stride, int64_t x_col_stride, double *Y,
                             int64_t y_row_stride, int64_t y_col_stride, int accumulate, const cmi_config *cfg, void *stream)
{
    return cmi::spmm_csr<double>(num_rows, num_cols, num_entries, Ap, Aj, Ax, k, X, x_row_stride, x_col_stride, Y, y_row_stride,
                                 y_col_stride, accumulate, cfg, stream);
}
CMI_API int cmi_spmm_csr_f32(int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *Ap, const int32_t *Aj,
                             const float *Ax, int64_t k, const float *X, int64_t x_row_stride, int64_t x_col_stride, float *Y,
                             int64_t y_row_stride, int64_t y_col_stride, int accumulate, const cmi_config *cfg, void *stream)
{
    return cmi::spmm_csr<float>(num_rows, num_cols, num_entries, Ap, Aj, Ax, k, X, x_row_stride, x_col_stride, Y, y_row_stride,
                                y_col_stride, accumulate, cfg, stream);
}
