// spmv_semiring.hip -- cusp::multiply(A, x, y, initialize, combine, reduce) on the device for the named functors of cusp/functional.h
// (DESIGN 3.16).  For every row i, in the matrix's value type, one rounding per operation (-ffp-contract=off):
//     s = y0 ? y0[i] : init_value;   for each entry of row i in the format's own order:   s = reduce(s, combine(A_ij, x_j));   y[i] = s
// The format's own order is that of cusp::detail::host_multiply: CSR storage order; COO the row's entries in storage order (entries sorted
// by row); ELL slots ascending, column -1 skipped; DIA diagonals in storage order, every in-range slot taking part, stored zeros included.
// minimum and maximum are `a < b ? a : b` and `a < b ? b : a`: with a NaN or a signed zero in the row they are neither commutative nor
// associative, so ONE lane runs a row's whole chain in order and no path joins partial results of two lanes.
// No kernel here allocates, synchronises or uses an atomic.  A stream the chosen operations do not need is not read: project2nd reads no
// matrix value, project1st reads no x (and, in CSR and COO, no column index).
#include "common.h"

namespace cmi {
namespace {

// combine(a, b): a the matrix value, b the vector value.  reduce(s, t): s the running value, t the new term.
struct op_plus       { template <typename T> static __device__ __forceinline__ T apply(T a, T b) { return a + b; } };
struct op_multiplies { template <typename T> static __device__ __forceinline__ T apply(T a, T b) { return a * b; } };
struct op_minimum    { template <typename T> static __device__ __forceinline__ T apply(T a, T b) { return a < b ? a : b; } };
struct op_maximum    { template <typename T> static __device__ __forceinline__ T apply(T a, T b) { return a < b ? b : a; } };
struct op_project1st { template <typename T> static __device__ __forceinline__ T apply(T a, T) { return a; } };
struct op_project2nd { template <typename T> static __device__ __forceinline__ T apply(T, T b) { return b; } };
template <typename C> constexpr bool reads_values = !std::is_same<C, op_project2nd>::value;
template <typename C> constexpr bool reads_vector = !std::is_same<C, op_project1st>::value;

// run f(Op()) for the runtime operation; false when `op` is none of the enum (or a projection where none may stand)
template <typename F> inline bool with_combine(int op, F &&f)
{
    switch (op) {
    case CMI_OP_PLUS: f(op_plus()); return true;
    case CMI_OP_MULTIPLIES: f(op_multiplies()); return true;
    case CMI_OP_MINIMUM: f(op_minimum()); return true;
    case CMI_OP_MAXIMUM: f(op_maximum()); return true;
    case CMI_OP_PROJECT1ST: f(op_project1st()); return true;
    case CMI_OP_PROJECT2ND: f(op_project2nd()); return true;
    default: return false;
    }
}
template <typename F> inline bool with_reduce(int op, F &&f)
{
    switch (op) {
    case CMI_OP_PLUS: f(op_plus()); return true;
    case CMI_OP_MULTIPLIES: f(op_multiplies()); return true;
    case CMI_OP_MINIMUM: f(op_minimum()); return true;
    case CMI_OP_MAXIMUM: f(op_maximum()); return true;
    default: return false;
    }
}

// s = reduce(s, p[0]), reduce(s, p[1]), ... in that order; the LDS reads of eight terms are issued before the first operation
// (common.h sum_in_order, with the operation a parameter)
template <typename R, typename T> __device__ __forceinline__ T chain_in_order(T s, const T *p, int n)
{
    int j = 0;
    for (; j + 8 <= n; j += 8) {
        const T v0 = p[j], v1 = p[j + 1], v2 = p[j + 2], v3 = p[j + 3], v4 = p[j + 4], v5 = p[j + 5], v6 = p[j + 6], v7 = p[j + 7];
        s = R::apply(s, v0); s = R::apply(s, v1); s = R::apply(s, v2); s = R::apply(s, v3);
        s = R::apply(s, v4); s = R::apply(s, v5); s = R::apply(s, v6); s = R::apply(s, v7);
    }
    for (; j < n; j++) s = R::apply(s, p[j]);
    return s;
}

// ---------------------------------------------------------------------------------------------
// CSR: the wave-private tile body of csr_wave_kernel (spmv_csr.hip, the plan-less form) with the two operations as types
// ---------------------------------------------------------------------------------------------
// Each 64-lane wave owns rows_per_wave (<= 64) consecutive rows: lane l requests entries l, l + 64, ..., l + 64 (K - 1) of the wave's tile,
// gathers x, parks combine(v, x[c]) in the wave's own LDS region, and row lane l runs its row's chain over the slots in storage order.  A
// tile of more than 64 K entries takes passes of 64 K, every row lane carrying its running value across them: a long row is one lane's
// serial chain, pass after pass (correct and slow, like the plan-less csr_wave).  No workgroup barrier: a wave's LDS
// instructions execute in order.  y0 may be y (a lane reads its own element before it writes it) or x, so neither is restrict.
// NT: the once-read index and value streams carry the nt hint (the host sets it beyond the Infinity Cache, plan.hip adopt_wave_shape's rule).
// LDS: T terms[waves][64 K].
template <typename T, int K, bool NT, typename C, typename R>
__global__ void __launch_bounds__(256)
csr_semiring_kernel(int64_t num_rows, const int *Ap, const int *__restrict__ Aj, const T *__restrict__ Ax, const T *x, const T *y0, T init,
                    T *y, int rows_per_wave, int64_t num_tiles, int64_t tiles_per_xcd, int swizzle)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int64_t tile = tile_of_block(blockIdx.x, tiles_per_xcd, swizzle);
    if (tile >= num_tiles) return; // whole workgroup
    const int waves = blockDim.x / kWave;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x & (kWave - 1);
    const int64_t r0 = (tile * waves + wave) * (int64_t)rows_per_wave;
    if (r0 >= num_rows) return; // whole wave; nothing below waits for another wave
    const int nr = (int)((num_rows - r0) < rows_per_wave ? (num_rows - r0) : rows_per_wave);
    const int nz0 = Ap[r0], nz1 = Ap[r0 + nr];
    const int cnt = nz1 - nz0;
    const int a = Ap[r0 + (lane < nr ? lane : nr)];
    const int b = __builtin_amdgcn_update_dpp(nz1, a, 0x130 /* wave_shl:1: the next lane's start; lane 63 keeps nz1 */, 0xf, 0xf, false);
    T s = init;
    if (y0 && lane < nr) s = y0[r0 + lane];
    T *mine = reinterpret_cast<T *>(smem) + (size_t)wave * kWave * K;
    if (cnt > 0 && cnt <= kWave * K) { // (uniform per wave)
        T v[K], xv[K];
#pragma unroll
        for (int k = 0; k < K; k++) { v[k] = T(0); xv[k] = T(0); }
        if constexpr (reads_vector<C>) {
            int c[K];
#pragma unroll
            for (int k = 0; k < K; k++) { const int i = k * kWave + lane; c[k] = ld<NT>(Aj + nz0 + (i < cnt ? i : 0)); }
            if constexpr (reads_values<C>) {
#pragma unroll
                for (int k = 0; k < K; k++) { const int i = k * kWave + lane; v[k] = ld<NT>(Ax + nz0 + (i < cnt ? i : 0)); }
            }
            __builtin_amdgcn_sched_barrier(0); // every stream request is out before the first gather address is formed
#pragma unroll
            for (int k = 0; k < K; k++) xv[k] = x[c[k]];
        } else {
#pragma unroll
            for (int k = 0; k < K; k++) { const int i = k * kWave + lane; v[k] = ld<NT>(Ax + nz0 + (i < cnt ? i : 0)); }
        }
#pragma unroll
        for (int k = 0; k < K; k++) mine[k * kWave + lane] = C::apply(v[k], xv[k]);
        __builtin_amdgcn_wave_barrier(); // (compiler only: the hardware runs a wave's LDS instructions in order)
        if (lane < nr) s = chain_in_order<R>(s, mine + (a - nz0), b - a);
    } else if (cnt > 0) {
        for (int base = nz0; base < nz1; base += kWave * K) {
            T t[K];
#pragma unroll
            for (int k = 0; k < K; k++) {
                const int i = base + k * kWave + lane;
                const int e = i < nz1 ? i : nz0;
                T v = T(0), xv = T(0);
                if constexpr (reads_values<C>) v = ld<NT>(Ax + e);
                if constexpr (reads_vector<C>) xv = x[ld<NT>(Aj + e)];
                t[k] = C::apply(v, xv);
            }
#pragma unroll
            for (int k = 0; k < K; k++) mine[k * kWave + lane] = t[k];
            __builtin_amdgcn_wave_barrier();
            if (lane < nr) {
                const int lo = a > base ? a : base, hi = b < base + kWave * K ? b : base + kWave * K;
                if (hi > lo) s = chain_in_order<R>(s, mine + (lo - base), hi - lo);
            }
            __builtin_amdgcn_wave_barrier(); // (the next pass overwrites the slots: in order behind these reads on the hardware)
        }
    }
    if (lane < nr) st<true>(y + r0 + lane, s); // (once-written: the streaming hint, as csr_wave's launch shape has it)
}

// ---------------------------------------------------------------------------------------------
// ELL, DIA, COO: one lane per row
// ---------------------------------------------------------------------------------------------
// ELL: slots ascending; a slot whose column is -1 is padding and takes no part (the column array is read whatever the operations are: it
// alone says which slots are padding).
template <typename T, typename C, typename R>
__global__ void __launch_bounds__(256)
ell_semiring_kernel(int64_t num_rows, int64_t num_cols, int64_t width, int64_t pitch, const int *__restrict__ Aj, const T *__restrict__ Ax,
                    const T *x, const T *y0, T init, T *y)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_rows) return;
    T s = y0 ? y0[i] : init;
    for (int64_t n = 0; n < width; n++) {
        const int64_t j = Aj[n * pitch + i];
        if (j < 0 || j >= num_cols) continue; // -1: padding (any other column outside the matrix is never used as an address)
        T v = T(0), xv = T(0);
        if constexpr (reads_values<C>) v = Ax[n * pitch + i];
        if constexpr (reads_vector<C>) xv = x[j];
        s = R::apply(s, C::apply(v, xv));
    }
    y[i] = s;
}

// DIA: diagonals in storage order; every slot whose column i + offset lies inside the matrix takes part, stored zeros included.
template <typename T, typename C, typename R>
__global__ void __launch_bounds__(256)
dia_semiring_kernel(int64_t num_rows, int64_t num_cols, int64_t num_diagonals, int64_t pitch, const int *__restrict__ offsets,
                    const T *__restrict__ values, const T *x, const T *y0, T init, T *y)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_rows) return;
    T s = y0 ? y0[i] : init;
    for (int64_t d = 0; d < num_diagonals; d++) {
        const int64_t j = i + (int64_t)offsets[d];
        if (j < 0 || j >= num_cols) continue;
        T v = T(0), xv = T(0);
        if constexpr (reads_values<C>) v = values[d * pitch + i];
        if constexpr (reads_vector<C>) xv = x[j];
        s = R::apply(s, C::apply(v, xv));
    }
    y[i] = s;
}

// COO, entries sorted by row: the row lane finds the first entry of its row by a binary search in Ai (the first position whose row index
// is not below i) and runs the chain while the row index is its own.  Row indices are compared, never used as addresses: on arrays that
// are not sorted the chains are unspecified and nothing is read or written out of bounds.
template <typename T, typename C, typename R>
__global__ void __launch_bounds__(256)
coo_semiring_kernel(int64_t num_rows, int64_t num_entries, const int *__restrict__ Ai, const int *__restrict__ Aj, const T *__restrict__ Ax,
                    const T *x, const T *y0, T init, T *y)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= num_rows) return;
    T s = y0 ? y0[i] : init;
    int64_t lo = 0, hi = num_entries;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (Ai[mid] < i) lo = mid + 1;
        else hi = mid;
    }
    for (int64_t e = lo; e < num_entries && Ai[e] == i; e++) {
        T v = T(0), xv = T(0);
        if constexpr (reads_values<C>) v = Ax[e];
        if constexpr (reads_vector<C>) xv = x[Aj[e]];
        s = R::apply(s, C::apply(v, xv));
    }
    y[i] = s;
}

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
inline bool is_combine(int op) { return op >= CMI_OP_PLUS && op <= CMI_OP_PROJECT2ND; }
inline bool is_reduce(int op) { return op >= CMI_OP_PLUS && op <= CMI_OP_MAXIMUM; }
inline bool overlap(const void *p, int64_t pn, const void *q, int64_t qn, size_t elem)
{
    if (!p || !q || pn <= 0 || qn <= 0) return false;
    const uintptr_t a = reinterpret_cast<uintptr_t>(p), b = reinterpret_cast<uintptr_t>(q);
    return a < b + (uintptr_t)qn * elem && b < a + (uintptr_t)pn * elem;
}

// what every entry point refuses before any device call; *done: nothing to launch
static int semiring_checks(const char *who, int64_t rows, int64_t cols, int64_t entries, int combine, int reduce, const void *x, const void *y,
                           size_t elem, bool *done)
{
    *done = false;
    if (!is_combine(combine)) { set_error("%s: combine is not a cmi_op", who); return CMI_ERROR_INVALID_VALUE; }
    if (!is_reduce(reduce)) { set_error("%s: reduce must be plus, multiplies, minimum or maximum (a projection cannot reduce)", who); return CMI_ERROR_INVALID_VALUE; }
    if (rows < 0 || cols < 0 || entries < 0) { set_error("%s: negative size", who); return CMI_ERROR_INVALID_VALUE; }
    if (rows > INT32_MAX || cols > INT32_MAX || entries > INT32_MAX - 65536) { set_error("%s: sizes exceed the int32 index type", who); return CMI_ERROR_INVALID_VALUE; }
    if (rows == 0) { *done = true; return CMI_SUCCESS; }
    if (!y) { set_error("%s: null y", who); return CMI_ERROR_INVALID_VALUE; }
    if (overlap(y, rows, x, cols, elem)) { set_error("%s: y overlaps x", who); return CMI_ERROR_INVALID_VALUE; }
    return CMI_SUCCESS;
}
inline int null_array(const char *who) { set_error("%s: null array that the chosen operations read", who); return CMI_ERROR_INVALID_VALUE; }
inline unsigned row_grid(int64_t rows) { return (unsigned)ceil_div(rows, 256); }

template <typename T>
static int csr_semiring(int64_t rows, int64_t cols, int64_t nnz, const int *Ap, const int *Aj, const T *Ax, const T *x, const T *y0, T init, int combine,
                        int reduce, T *y, void *stream)
{
    const char *who = "cmi_spmv_csr_semiring";
    bool done;
    if (int st = semiring_checks(who, rows, cols, nnz, combine, reduce, x, y, sizeof(T), &done)) return st;
    if (done) return CMI_SUCCESS;
    const bool needs_values = combine != CMI_OP_PROJECT2ND, needs_vector = combine != CMI_OP_PROJECT1ST;
    if (!Ap || (nnz > 0 && ((needs_values && !Ax) || (needs_vector && (!Aj || !x))))) return null_array(who);
    // The launch shape from the sizes alone (no device read): K entries per lane, the smallest of 2 / 5 / 8 that holds the mean row, and as
    // many rows per wave (<= 64) as fill the wave's 64 K slots at that mean.  A stencil's tile then takes one pass; whatever does not fit
    // takes further passes.
    const double mean = (double)nnz / (double)rows;
    const int K = mean <= 2.0 ? 2 : mean <= 5.0 ? 5 : 8;
    int rpw = kWave;
    if (mean > (double)K) {
        rpw = (int)((double)(kWave * K) / mean);
        rpw = rpw < 1 ? 1 : rpw > kWave ? kWave : rpw;
    }
    constexpr int block = 256, waves = block / kWave;
    // What the plan-less csr_wave launch takes from the table and from adopt_wave_shape (plan.hip), taken the same way: the CSR bucket's XCD
    // dealing, and the nt hint on the once-read streams when they do not fit the Infinity Cache (the streams this combine reads).
    cmi_config table;
    select_config(CMI_FORMAT_CSR, std::is_same<T, double>::value ? CMI_F64 : CMI_F32, rows, cols, nnz, nullptr, &table);
    const int64_t bytes_per_entry = (needs_vector ? (int64_t)sizeof(int) : 0) + (needs_values ? (int64_t)sizeof(T) : 0);
    const bool nt = nnz * bytes_per_entry > kInfinityCacheBytes + kInfinityCacheBytes / 4;
    tile_launch g;
    if (int st = tile_launch_for(ceil_div(rows, (int64_t)rpw * waves), table.xcd_swizzle, who, &g)) return st;
    const size_t lds = (size_t)block * K * sizeof(T);
    with_int<2, 5, 8>(K, [&](auto KK) {
        with_bool(nt, [&](auto NT) {
            with_combine(combine, [&](auto C) {
                with_reduce(reduce, [&](auto R) {
                    hipLaunchKernelGGL((csr_semiring_kernel<T, decltype(KK)::value, decltype(NT)::value, decltype(C), decltype(R)>), dim3(g.grid), dim3(block), lds,
                                       as_stream(stream), rows, Ap, Aj, Ax, x, y0, init, y, rpw, g.tiles, g.tiles_per_xcd, g.swizzle);
                });
            });
        });
    });
    CMI_LAUNCH_CHECK("csr semiring spmv");
    return CMI_SUCCESS;
}

template <typename T>
static int ell_semiring(int64_t rows, int64_t cols, int64_t width, int64_t pitch, const int *Aj, const T *Ax, const T *x, const T *y0, T init, int combine,
                        int reduce, T *y, void *stream)
{
    const char *who = "cmi_spmv_ell_semiring";
    bool done;
    if (int st = semiring_checks(who, rows, cols, width, combine, reduce, x, y, sizeof(T), &done)) return st;
    if (done) return CMI_SUCCESS;
    if (pitch < rows) { set_error("%s: pitch is smaller than num_rows", who); return CMI_ERROR_INVALID_VALUE; }
    if (width > 0 && (!Aj || (combine != CMI_OP_PROJECT2ND && !Ax) || (combine != CMI_OP_PROJECT1ST && !x))) return null_array(who);
    with_combine(combine, [&](auto C) {
        with_reduce(reduce, [&](auto R) {
            hipLaunchKernelGGL((ell_semiring_kernel<T, decltype(C), decltype(R)>), dim3(row_grid(rows)), dim3(256), 0, as_stream(stream), rows, cols, width, pitch,
                               Aj, Ax, x, y0, init, y);
        });
    });
    CMI_LAUNCH_CHECK("ell semiring spmv");
    return CMI_SUCCESS;
}

template <typename T>
static int dia_semiring(int64_t rows, int64_t cols, int64_t nd, int64_t pitch, const int *offsets, const T *values, const T *x, const T *y0, T init,
                        int combine, int reduce, T *y, void *stream)
{
    const char *who = "cmi_spmv_dia_semiring";
    bool done;
    if (int st = semiring_checks(who, rows, cols, nd, combine, reduce, x, y, sizeof(T), &done)) return st;
    if (done) return CMI_SUCCESS;
    if (pitch < rows) { set_error("%s: pitch is smaller than num_rows", who); return CMI_ERROR_INVALID_VALUE; }
    if (nd > 0 && (!offsets || (combine != CMI_OP_PROJECT2ND && !values) || (combine != CMI_OP_PROJECT1ST && !x))) return null_array(who);
    with_combine(combine, [&](auto C) {
        with_reduce(reduce, [&](auto R) {
            hipLaunchKernelGGL((dia_semiring_kernel<T, decltype(C), decltype(R)>), dim3(row_grid(rows)), dim3(256), 0, as_stream(stream), rows, cols, nd, pitch,
                               offsets, values, x, y0, init, y);
        });
    });
    CMI_LAUNCH_CHECK("dia semiring spmv");
    return CMI_SUCCESS;
}

template <typename T>
static int coo_semiring(int64_t rows, int64_t cols, int64_t nnz, const int *Ai, const int *Aj, const T *Ax, const T *x, const T *y0, T init, int combine,
                        int reduce, T *y, void *stream)
{
    const char *who = "cmi_spmv_coo_semiring";
    bool done;
    if (int st = semiring_checks(who, rows, cols, nnz, combine, reduce, x, y, sizeof(T), &done)) return st;
    if (done) return CMI_SUCCESS;
    const bool needs_values = combine != CMI_OP_PROJECT2ND, needs_vector = combine != CMI_OP_PROJECT1ST;
    if (nnz > 0 && (!Ai || (needs_values && !Ax) || (needs_vector && (!Aj || !x)))) return null_array(who);
    with_combine(combine, [&](auto C) {
        with_reduce(reduce, [&](auto R) {
            hipLaunchKernelGGL((coo_semiring_kernel<T, decltype(C), decltype(R)>), dim3(row_grid(rows)), dim3(256), 0, as_stream(stream), rows, nnz, Ai, Aj, Ax, x,
                               y0, init, y);
        });
    });
    CMI_LAUNCH_CHECK("coo semiring spmv");
    return CMI_SUCCESS;
}

} // namespace
} // namespace cmi

CMI_API int cmi_spmv_csr_semiring_f64(int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *Ap, const int32_t *Aj, const double *Ax,
                                      const double *x, const double *y0, double init_value, int combine, int reduce, double *y, void *stream)
{
    return cmi::csr_semiring<double>(num_rows, num_cols, num_entries, Ap, Aj, Ax, x, y0, init_value, combine, reduce, y, stream);
}
CMI_API int cmi_spmv_csr_semiring_f32(int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *Ap, const int32_t *Aj, const float *Ax,
                                      const float *x, const float *y0, float init_value, int combine, int reduce, float *y, void *stream)
{
    return cmi::csr_semiring<float>(num_rows, num_cols, num_entries, Ap, Aj, Ax, x, y0, init_value, combine, reduce, y, stream);
}
CMI_API int cmi_spmv_ell_semiring_f64(int64_t num_rows, int64_t num_cols, int64_t num_entries_per_row, int64_t pitch, const int32_t *Aj, const double *Ax,
                                      const double *x, const double *y0, double init_value, int combine, int reduce, double *y, void *stream)
{
    return cmi::ell_semiring<double>(num_rows, num_cols, num_entries_per_row, pitch, Aj, Ax, x, y0, init_value, combine, reduce, y, stream);
}
CMI_API int cmi_spmv_ell_semiring_f32(int64_t num_rows, int64_t num_cols, int64_t num_entries_per_row, int64_t pitch, const int32_t *Aj, const float *Ax,
                                      const float *x, const float *y0, float init_value, int combine, int reduce, float *y, void *stream)
{
    return cmi::ell_semiring<float>(num_rows, num_cols, num_entries_per_row, pitch, Aj, Ax, x, y0, init_value, combine, reduce, y, stream);
}
CMI_API int cmi_spmv_dia_semiring_f64(int64_t num_rows, int64_t num_cols, int64_t num_diagonals, int64_t pitch, const int32_t *diagonal_offsets,
                                      const double *values, const double *x, const double *y0, double init_value, int combine, int reduce, double *y,
                                      void *stream)
{
    return cmi::dia_semiring<double>(num_rows, num_cols, num_diagonals, pitch, diagonal_offsets, values, x, y0, init_value, combine, reduce, y, stream);
}
CMI_API int cmi_spmv_dia_semiring_f32(int64_t num_rows, int64_t num_cols, int64_t num_diagonals, int64_t pitch, const int32_t *diagonal_offsets,
                                      const float *values, const float *x, const float *y0, float init_value, int combine, int reduce, float *y, void *stream)
{
    return cmi::dia_semiring<float>(num_rows, num_cols, num_diagonals, pitch, diagonal_offsets, values, x, y0, init_value, combine, reduce, y, stream);
}
CMI_API int cmi_spmv_coo_semiring_f64(int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *Ai, const int32_t *Aj, const double *Ax,
                                      const double *x, const double *y0, double init_value, int combine, int reduce, double *y, void *stream)
{
    return cmi::coo_semiring<double>(num_rows, num_cols, num_entries, Ai, Aj, Ax, x, y0, init_value, combine, reduce, y, stream);
}
CMI_API int cmi_spmv_coo_semiring_f32(int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *Ai, const int32_t *Aj, const float *Ax,
                                      const float *x, const float *y0, float init_value, int combine, int reduce, float *y, void *stream)
{
    return cmi::coo_semiring<float>(num_rows, num_cols, num_entries, Ai, Aj, Ax, x, y0, init_value, combine, reduce, y, stream);
}
