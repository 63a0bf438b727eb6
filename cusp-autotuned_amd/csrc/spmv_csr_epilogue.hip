// spmv_csr_epilogue.hip -- a CSR row sweep whose write-back is a fixed elementwise expression: the two smoothers that
// are "an SpMV, then one or two passes over the vector it just wrote" (reference cusp/relaxation/detail/jacobi.inl:77-87,
// polynomial.inl:117-142), in one launch and without the intermediate vector.
//
// The row sum is the host loop's (sequential/multiply/csr_spmv.h):
//   s_i = (((T(0) + Ax[j0] * x[Aj[j0]]) + Ax[j0 + 1] * x[Aj[j0 + 1]]) + ...)   in storage order, by ONE lane,
// multiply, then add (-ffp-contract=off), i.e. the bits of cmi_spmv_csr_* through any of its storage-order kernels.
// The lane that owns row i then evaluates, once,
//   axpby form   out[i]   = alpha * s_i + beta * z[i]                  (out may be z: the lane reads only its own z[i])
//   Jacobi form  x_out[i] = x[i] + omega * (b[i] - s_i) / diag[i]      (omega * (b - s) first, then the division)
// and stores one value with a plain vector store.  No atomics, no allocation, no synchronisation.
//
// Tiling (its own; a plan is checked and otherwise not needed -- every valid CSR plan class is accepted): a workgroup of
// kEpiBlock = 256 lanes owns kEpiBlock consecutive rows, one lane per row.  The rows' entries are one contiguous span of
// (Aj, Ax); it is streamed through LDS in passes of kEpiChunk entries: every lane takes groups of four consecutive
// entries (one 16-byte load of Aj, two (f64) or one (f32) of Ax where the arrays are 16-byte aligned and the group lies
// inside the span; scalar loads at the span's two ragged ends and for unaligned arrays), gathers x and parks the four
// products; after a barrier lane r adds the products of row r that the pass holds, in order.  A row of any length just
// takes more passes; an empty row adds nothing and its lane evaluates the epilogue on s = 0.  z / b / diag / x[i] and the
// store are one element per lane, consecutive lanes on consecutive addresses.
#include "common.h"

namespace cmi {

constexpr int kEpiBlock = 256;  // lanes = rows per workgroup
constexpr int kEpiChunk = 2048; // entries per LDS pass: 16 KiB (f64) / 8 KiB (f32)
constexpr int kEpiAxpby = 0, kEpiJacobi = 1;

// FORM kEpiAxpby:  p0 = alpha, p1 = beta,  u = z,  v unused.   FORM kEpiJacobi: p0 = omega, u = b, v = diag.
template <typename T, int FORM, bool VEC>
__global__ void __launch_bounds__(kEpiBlock)
csr_epilogue_kernel(int64_t num_rows, const int *__restrict__ Ap, const int *__restrict__ Aj, const T *__restrict__ Ax,
                    const T *__restrict__ x, T p0, T p1, const T *u, const T *__restrict__ v, T *out)
{
    __shared__ __attribute__((aligned(16))) T prod[kEpiChunk];
    const int tid = threadIdx.x;
    const int64_t r0 = (int64_t)blockIdx.x * kEpiBlock;
    const int nr = (int)(num_rows - r0 < kEpiBlock ? num_rows - r0 : kEpiBlock);
    const bool has_row = tid < nr;
    const int e0 = Ap[r0], e1 = Ap[r0 + nr]; // uniform
    const int a = Ap[r0 + (has_row ? tid : nr)], b = Ap[r0 + (has_row ? tid + 1 : nr)];

    // the epilogue's operands: requested before the streams, needed after the last pass
    T uv = T(0), vv = T(1), xv = T(0);
    if (has_row) {
        uv = u[r0 + tid];
        if constexpr (FORM == kEpiJacobi) { vv = v[r0 + tid]; xv = x[r0 + tid]; }
    }

    T s = T(0);
    for (int base = e0 & ~3; base < e1; base += kEpiChunk) { // (base + kEpiChunk stays inside int: the CSR ceiling)
        if (base != (e0 & ~3)) __syncthreads();              // every lane has read the previous pass
        for (int slot = tid * 4; slot < kEpiChunk; slot += kEpiBlock * 4) {
            const int e = base + slot;
            if (e >= e1) break;
            if (VEC && e >= e0 && e + 4 <= e1) {
                const int4v c = *reinterpret_cast<const int4v *>(Aj + e);
                T a0, a1, a2, a3;
                if constexpr (sizeof(T) == 8) {
                    const double2v v01 = *reinterpret_cast<const double2v *>(Ax + e);
                    const double2v v23 = *reinterpret_cast<const double2v *>(Ax + e + 2);
                    a0 = v01.x; a1 = v01.y; a2 = v23.x; a3 = v23.y;
                } else {
                    const float4v v4 = *reinterpret_cast<const float4v *>(Ax + e);
                    a0 = v4.x; a1 = v4.y; a2 = v4.z; a3 = v4.w;
                }
                const T x0 = x[c.x], x1 = x[c.y], x2 = x[c.z], x3 = x[c.w];
                prod[slot + 0] = a0 * x0; prod[slot + 1] = a1 * x1;
                prod[slot + 2] = a2 * x2; prod[slot + 3] = a3 * x3;
            } else {
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const int j = e + q;
                    if (j >= e0 && j < e1) prod[slot + q] = Ax[j] * x[Aj[j]];
                }
            }
        }
        __syncthreads();
        if (has_row) {
            const int lo = a > base ? a : base;
            const int hi = b < base + kEpiChunk ? b : base + kEpiChunk;
            if (hi > lo) s = sum_in_order(s, prod + (lo - base), hi - lo);
        }
    }
    if (!has_row) return;
    T r;
    if constexpr (FORM == kEpiAxpby) {
        const T t0 = p0 * s, t1 = p1 * uv;
        r = t0 + t1;
    } else {
        const T d = uv - s;
        const T t = p0 * d;
        r = xv + t / vv;
    }
    out[r0 + tid] = r;
}

// x[i] = x[i] + omega * (b[i] - y[i]) / diag[i], in place: the Jacobi update behind a multiply of any format
template <typename T>
__global__ void __launch_bounds__(256) jacobi_update_kernel(int64_t n, const T *__restrict__ diag, const T *__restrict__ b,
                                                            const T *__restrict__ y, T omega, T *__restrict__ x)
{
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const T d = b[i] - y[i];
        const T t = omega * d;
        x[i] = x[i] + t / diag[i];
    }
}

static bool ranges_overlap(const void *p, int64_t np, const void *q, int64_t nq, size_t s)
{
    const uintptr_t pl = reinterpret_cast<uintptr_t>(p), ph = pl + (uintptr_t)np * s;
    const uintptr_t ql = reinterpret_cast<uintptr_t>(q), qh = ql + (uintptr_t)nq * s;
    return np > 0 && nq > 0 && pl < qh && ql < ph;
}

// the checks both forms share; *done: nothing to launch
template <typename T>
static int epilogue_check(const char *who, int dtype, const cmi_plan *plan, int64_t rows, int64_t cols, int64_t nnz, const int *Ap,
                          const int *Aj, const T *Ax, const T *x, const T *out, bool *done)
{
    *done = false;
    if (rows < 0 || cols < 0 || nnz < 0) { set_error("%s: negative size", who); return CMI_ERROR_INVALID_VALUE; }
    if (rows > INT32_MAX || cols > INT32_MAX || nnz > INT32_MAX - 65536) {
        set_error("%s: sizes exceed the int32 index type", who);
        return CMI_ERROR_INVALID_VALUE;
    }
    if (plan && (plan->format != CMI_FORMAT_CSR || plan->dtype != dtype)) {
        set_error("%s: the plan was made for another format or value type", who);
        return CMI_ERROR_INVALID_VALUE;
    }
    if (rows == 0) { *done = true; return CMI_SUCCESS; }
    if (!Ap || !out || (nnz > 0 && (!Aj || !Ax)) || (cols > 0 && !x)) { set_error("%s: null array", who); return CMI_ERROR_INVALID_VALUE; }
    if (ranges_overlap(out, rows, x, cols, sizeof(T))) { set_error("%s: the output overlaps x", who); return CMI_ERROR_INVALID_VALUE; }
    return CMI_SUCCESS;
}

template <typename T, int FORM>
static int epilogue_launch(int64_t rows, const int *Ap, const int *Aj, const T *Ax, const T *x, T p0, T p1, const T *u, const T *v, T *out,
                           void *stream)
{
    const bool vec = aligned16(Aj, Ax);
    const dim3 grid((unsigned)ceil_div(rows, kEpiBlock)); // rows <= INT32_MAX
    with_bool(vec, [&](auto VEC) {
        hipLaunchKernelGGL((csr_epilogue_kernel<T, FORM, decltype(VEC)::value>), grid, dim3(kEpiBlock), 0, as_stream(stream), rows, Ap, Aj, Ax,
                           x, p0, p1, u, v, out);
    });
    CMI_LAUNCH_CHECK("csr epilogue sweep");
    return CMI_SUCCESS;
}

template <typename T>
static int spmv_csr_axpby(int dtype, const cmi_plan *plan, int64_t rows, int64_t cols, int64_t nnz, const int *Ap, const int *Aj, const T *Ax,
                          const T *x, T alpha, T beta, const T *z, T *out, void *stream)
{
    bool done;
    if (int st = epilogue_check("cmi_spmv_csr_axpby", dtype, plan, rows, cols, nnz, Ap, Aj, Ax, x, out, &done)) return st;
    if (done) return CMI_SUCCESS;
    if (!z) return fail(CMI_ERROR_INVALID_VALUE, "cmi_spmv_csr_axpby: null array");
    return epilogue_launch<T, kEpiAxpby>(rows, Ap, Aj, Ax, x, alpha, beta, z, nullptr, out, stream);
}

template <typename T>
static int csr_jacobi_sweep(int dtype, const cmi_plan *plan, int64_t rows, int64_t nnz, const int *Ap, const int *Aj, const T *Ax,
                            const T *diag, const T *b, const T *x, T omega, T *x_out, void *stream)
{
    bool done;
    if (int st = epilogue_check("cmi_csr_jacobi_sweep", dtype, plan, rows, rows, nnz, Ap, Aj, Ax, x, x_out, &done)) return st;
    if (done) return CMI_SUCCESS;
    if (!diag || !b) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_jacobi_sweep: null array");
    if (ranges_overlap(x_out, rows, diag, rows, sizeof(T)) || ranges_overlap(x_out, rows, b, rows, sizeof(T)))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_jacobi_sweep: the output overlaps diag or b");
    return epilogue_launch<T, kEpiJacobi>(rows, Ap, Aj, Ax, x, omega, T(0), b, diag, x_out, stream);
}

template <typename T> static int relax_jacobi_update(int64_t n, const T *diag, const T *b, const T *y, T omega, T *x, void *stream)
{
    if (n < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_relax_jacobi_update: negative n");
    if (n == 0) return CMI_SUCCESS;
    if (!diag || !b || !y || !x) return fail(CMI_ERROR_INVALID_VALUE, "cmi_relax_jacobi_update: null array");
    if (ranges_overlap(x, n, y, n, sizeof(T)) || ranges_overlap(x, n, b, n, sizeof(T)) || ranges_overlap(x, n, diag, n, sizeof(T)))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_relax_jacobi_update: x overlaps an input");
    const int64_t blocks = ceil_div(n, 256), cap = (int64_t)kCus * 8;
    hipLaunchKernelGGL((jacobi_update_kernel<T>), dim3((unsigned)(blocks < cap ? blocks : cap)), dim3(256), 0, as_stream(stream), n, diag, b, y,
                       omega, x);
    CMI_LAUNCH_CHECK("jacobi update");
    return CMI_SUCCESS;
}

} // namespace cmi

CMI_API int cmi_spmv_csr_axpby_f64(const cmi_plan *plan, int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *Ap,
                                   const int32_t *Aj, const double *Ax, const double *x, double alpha, double beta, const double *z,
                                   double *out, void *stream)
{
    return cmi::spmv_csr_axpby<double>(CMI_F64, plan, num_rows, num_cols, num_entries, Ap, Aj, Ax, x, alpha, beta, z, out, stream);
}
CMI_API int cmi_spmv_csr_axpby_f32(const cmi_plan *plan, int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *Ap,
                                   const int32_t *Aj, const float *Ax, const float *x, float alpha, float beta, const float *z, float *out,
                                   void *stream)
{
    return cmi::spmv_csr_axpby<float>(CMI_F32, plan, num_rows, num_cols, num_entries, Ap, Aj, Ax, x, alpha, beta, z, out, stream);
}
CMI_API int cmi_csr_jacobi_sweep_f64(const cmi_plan *plan, int64_t num_rows, int64_t num_entries, const int32_t *Ap, const int32_t *Aj,
                                     const double *Ax, const double *diag, const double *b, const double *x, double omega, double *x_out,
                                     void *stream)
{
    return cmi::csr_jacobi_sweep<double>(CMI_F64, plan, num_rows, num_entries, Ap, Aj, Ax, diag, b, x, omega, x_out, stream);
}
CMI_API int cmi_csr_jacobi_sweep_f32(const cmi_plan *plan, int64_t num_rows, int64_t num_entries, const int32_t *Ap, const int32_t *Aj,
                                     const float *Ax, const float *diag, const float *b, const float *x, float omega, float *x_out,
                                     void *stream)
{
    return cmi::csr_jacobi_sweep<float>(CMI_F32, plan, num_rows, num_entries, Ap, Aj, Ax, diag, b, x, omega, x_out, stream);
}
CMI_API int cmi_relax_jacobi_update_f64(int64_t n, const double *diag, const double *b, const double *y, double omega, double *x, void *stream)
{
    return cmi::relax_jacobi_update<double>(n, diag, b, y, omega, x, stream);
}
CMI_API int cmi_relax_jacobi_update_f32(int64_t n, const float *diag, const float *b, const float *y, float omega, float *x, void *stream)
{
    return cmi::relax_jacobi_update<float>(n, diag, b, y, omega, x, stream);
}
