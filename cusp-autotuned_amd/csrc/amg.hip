// amg.hip -- the set-up kernels of smoothed-aggregation multigrid: strength filter, row scaling, tentative
// prolongator, CSR +/- CSR, Jacobi presmoothing.
//
// Replaces (reference): cusp/precond/aggregation/system/detail/sequential/symmetric_strength.h (two passes over A),
// .../sequential/smooth_prolongator.h:65-76 (the division loop and blas::scal), .../generic/tentative.h (copy_if, transpose,
// reduce_by_key, two transforms), cusp/system/detail/sequential/elementwise.h (add / subtract) and the
// jacobi_presmooth_functor of cusp/relaxation/detail/jacobi.inl.
//
// Contract shared by all of them: the bits of the sequential loops as include/cusp_mi355x.h states them.  Every value is
// produced by ONE lane in a fixed order; no atomics (device flags are plain stores of the same word); multiply, divide, add and
// square root are rounded separately (-ffp-contract=off, correctly rounded division and square root).  Every output is
// bounded by its inputs: the caller allocates the bound, the call compacts into it.  The calls with a compaction allocate
// scratch, release it on every path out and synchronise the stream (as cmi_spgemm_csr_* does); scale_rows and
// jacobi_presmooth allocate nothing and do not synchronise.
//
// Bad offsets are the caller's error, but none addresses memory unclamped: row offsets are clamped to [0, num_entries], a
// decreasing pair is an empty row, a column outside the matrix reads no diagonal, and no lane writes at or beyond `capacity`.
#include "amg_shared.h"

namespace cmi {

// correctly rounded: the plain functions (the compiler's IEEE square root; hipcc's default is the correctly rounded f32 divide and
// square root).  The _rn intrinsics are NOT: without OCML's rounded-operations switch __fsqrt_rn is the native, 1-ulp instruction.
__device__ __forceinline__ double amg_sqrt(double v) { return sqrt(v); }
__device__ __forceinline__ float amg_sqrt(float v) { return sqrtf(v); }
__device__ __forceinline__ double amg_abs(double v) { return fabs(v); }
__device__ __forceinline__ float amg_abs(float v) { return fabsf(v); }

// ---- (a) symmetric strength of connection ---------------------------------------------------------------------------------
// |A_ij| >= theta * sqrt(|A_ii| |A_jj|): product and square root in T, the product with theta and the comparison in double
// (symmetric_strength.h:72 with its `const double theta`).  A NaN on either side compares false: the entry is dropped.
template <typename T> __device__ __forceinline__ bool amg_strong(T aij, T aii, T ajj, double theta)
{
    const T prod = amg_abs(aii) * amg_abs(ajj);
    const T root = amg_sqrt(prod);
    return (double)amg_abs(aij) >= theta * (double)root;
}

// One wave per 64 consecutive rows.  A row of at most 64 entries is walked by its own lane; a longer row by the whole wave,
// 64 entries at a time: a ballot of the predicate, its popcount is the chunk's count and the popcount below a lane that
// lane's place, so storage order is preserved.  FILL == false: count[i] = entries kept in row i (count[num_rows] = 0).
// FILL == true: the kept entries of row i are written from Sp[i] on.
template <typename T, bool FILL>
__global__ void __launch_bounds__(kAmgBlock)
strength_kernel(int64_t num_rows, int64_t num_entries, const int *__restrict__ Ap, const int *__restrict__ Aj, const T *__restrict__ Ax,
                const T *__restrict__ diag, double theta, int *__restrict__ count, const int *__restrict__ Sp, int *__restrict__ Sj,
                T *__restrict__ Sx, int64_t capacity)
{
    const int64_t row = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x; // (block = 4 waves of 64 consecutive rows each)
    const int lane = threadIdx.x & (kWave - 1);
    int lo = 0, hi = 0;
    T aii = T(0);
    if (row < num_rows) {
        lo = amg_clamp(Ap[row], num_entries);
        hi = amg_clamp(Ap[row + 1], num_entries);
        if (hi < lo) hi = lo;
        aii = diag[row];
    }
    int64_t out = 0;
    if (FILL && row < num_rows) out = Sp[row];
    const bool is_long = hi - lo > kWave;
    int kept = 0;
    if (!is_long) {
        for (int jj = lo; jj < hi; jj++) {
            const int j = Aj[jj];
            const T aij = Ax[jj];
            const T ajj = (j >= 0 && (int64_t)j < num_rows) ? diag[j] : T(0);
            if (amg_strong(aij, aii, ajj, theta)) {
                if (FILL && out + kept < capacity) {
                    Sj[out + kept] = j;
                    Sx[out + kept] = aij;
                }
                kept++;
            }
        }
    }
    unsigned long long todo = __ballot(is_long); // every lane of the wave is here: no lane has left
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const int rlo = __shfl(lo, src), rhi = __shfl(hi, src);
        const T raii = __shfl(aii, src);
        const int64_t rout = FILL ? __shfl(out, src) : 0;
        int n = 0;
        for (int base = rlo; base < rhi; base += kWave) {
            const int jj = base + lane; // (rhi <= INT32_MAX - 65536: no overflow)
            bool keep = false;
            int j = 0;
            T aij = T(0);
            if (jj < rhi) {
                j = Aj[jj];
                aij = Ax[jj];
                const T ajj = (j >= 0 && (int64_t)j < num_rows) ? diag[j] : T(0);
                keep = amg_strong(aij, raii, ajj, theta);
            }
            const unsigned long long mask = __ballot(keep);
            if (FILL && keep) {
                const int64_t at = rout + n + __popcll(mask & ((1ull << lane) - 1ull));
                if (at < capacity) {
                    Sj[at] = j;
                    Sx[at] = aij;
                }
            }
            n += __popcll(mask);
        }
        if (lane == src) kept = n;
    }
    if (!FILL) {
        if (row < num_rows) count[row] = kept;
        else if (row == num_rows) count[row] = 0;
    }
}

// diag[i] = the storage-order sum (from 0) of row i's entries in column i, 0 when none is stored: what cmi_csr_diagonal_* gives
// (cusp::extract_diagonal), restated here with the row offsets CLAMPED, so that a bad offset reads nothing outside the arrays
template <typename T>
__global__ void __launch_bounds__(kAmgBlock)
strength_diagonal_kernel(int64_t num_rows, int64_t num_entries, const int *__restrict__ Ap, const int *__restrict__ Aj, const T *__restrict__ Ax, T *__restrict__ diag)
{
    const int64_t row = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (row >= num_rows) return;
    const int lo = amg_clamp(Ap[row], num_entries), hi = amg_clamp(Ap[row + 1], num_entries);
    T d = T(0);
    for (int jj = lo; jj < hi; jj++)
        if ((int64_t)Aj[jj] == row) d += Ax[jj];
    diag[row] = d;
}

template <typename T>
static int strength_symmetric(int64_t num_rows, int64_t num_cols, int64_t num_entries, const int *Ap, const int *Aj, const T *Ax, double theta, int *Sp,
                              int *Sj, T *Sx, int64_t capacity, void *stream)
{
    if (num_rows < 0 || num_cols < 0 || num_entries < 0 || capacity < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_strength_symmetric: negative size");
    if (num_rows > INT32_MAX - 1 || num_cols > INT32_MAX - 1 || num_entries > kAmgCeiling)
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_strength_symmetric: sizes exceed the int32 index type");
    if (num_rows != num_cols) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_strength_symmetric: the matrix must be square");
    if (capacity < num_entries) {
        set_error("cmi_csr_strength_symmetric: capacity %lld is below the %lld entries of A", (long long)capacity, (long long)num_entries);
        return CMI_ERROR_INVALID_VALUE;
    }
    if (!Sp || (num_rows > 0 && !Ap) || (num_entries > 0 && (!Aj || !Ax || !Sj || !Sx))) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_strength_symmetric: null array");
    hipStream_t s = as_stream(stream);
    if (num_rows == 0 || num_entries == 0) { // nothing to keep: an all-zero Sp
        CMI_HIP(hipMemsetAsync(Sp, 0, (size_t)(num_rows + 1) * sizeof(int), s));
        CMI_HIP(hipStreamSynchronize(s));
        return CMI_SUCCESS;
    }
    device_array<T> diag_block;
    device_array<int> count_block;
    device_array<unsigned char> scan_temp;
    hipError_t e = diag_block.alloc((size_t)num_rows);
    if (e == hipSuccess) e = count_block.alloc((size_t)num_rows + 1);
    if (e != hipSuccess) return hip_fail(e, "cmi_csr_strength_symmetric: scratch");
    T *const diag = diag_block.get();
    int *const count = count_block.get();
    int st = CMI_SUCCESS;
    e = launch(strength_diagonal_kernel<T>, amg_blocks(num_rows), kAmgBlock, 0, s, num_rows, num_entries, Ap, Aj, Ax, diag);
    if (e != hipSuccess) st = hip_fail(e, "launch strength diagonal");
    if (st == CMI_SUCCESS) {
        e = launch(strength_kernel<T, false>, amg_blocks(num_rows + 1), kAmgBlock, 0, s, num_rows, num_entries, Ap, Aj, Ax, diag, theta, count, nullptr, nullptr,
                   nullptr, capacity);
        if (e == hipSuccess) e = exclusive_offsets(scan_temp, count, Sp, num_rows, s);
        if (e == hipSuccess)
            e = launch(strength_kernel<T, true>, amg_blocks(num_rows), kAmgBlock, 0, s, num_rows, num_entries, Ap, Aj, Ax, diag, theta, nullptr, Sp, Sj, Sx, capacity);
        if (e != hipSuccess) st = hip_fail(e, "cmi_csr_strength_symmetric");
    }
    // the scratch is released when this returns: everything enqueued above must have finished with it
    e = hipStreamSynchronize(s);
    if (st == CMI_SUCCESS && e != hipSuccess) st = hip_fail(e, "cmi_csr_strength_symmetric");
    return st;
}

// ---- (b) out[e] = (Ax[e] / d[row(e)]) * lambda -------------------------------------------------------------------------------
// One lane per ENTRY; its row is the largest i with Ap[i] <= e (empty rows share their successor's offset and lose).
template <typename T>
__global__ void __launch_bounds__(kAmgBlock)
scale_rows_kernel(int64_t num_rows, int64_t num_entries, const int *__restrict__ Ap, const T *Ax, const T *__restrict__ d, T lambda, T *out)
{
    const int64_t e = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (e >= num_entries) return;
    int64_t lo = 0, hi = num_rows - 1;
    while (lo < hi) {
        const int64_t mid = (lo + hi + 1) >> 1;
        if ((int64_t)Ap[mid] <= e) lo = mid;
        else hi = mid - 1;
    }
    const T q = Ax[e] / d[lo];
    out[e] = q * lambda;
}

template <typename T> static int scale_rows(int64_t num_rows, int64_t num_entries, const int *Ap, const T *Ax, const T *d, T lambda, T *out, void *stream)
{
    if (num_rows < 0 || num_entries < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_scale_rows: negative size");
    if (num_rows > INT32_MAX - 1 || num_entries > kAmgCeiling) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_scale_rows: sizes exceed the int32 index type");
    if (num_entries > 0 && num_rows == 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_scale_rows: entries without rows");
    if (num_entries > 0 && (!Ap || !Ax || !d || !out)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_scale_rows: null array");
    if (num_entries == 0) return CMI_SUCCESS;
    hipLaunchKernelGGL((scale_rows_kernel<T>), dim3(amg_blocks(num_entries)), dim3(kAmgBlock), 0, as_stream(stream), num_rows, num_entries, Ap, Ax, d, lambda, out);
    CMI_LAUNCH_CHECK("csr_scale_rows");
    return CMI_SUCCESS;
}

// ---- (e) x[i] = (omega * b[i]) / d[i] ----------------------------------------------------------------------------------------
template <typename T>
__global__ void __launch_bounds__(kAmgBlock) jacobi_presmooth_kernel(int64_t n, const T *__restrict__ d, const T *__restrict__ b, T omega, T *__restrict__ x)
{
    const int64_t i = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (i >= n) return;
    const T p = omega * b[i];
    x[i] = p / d[i];
}

template <typename T> static int jacobi_presmooth(int64_t n, const T *d, const T *b, T omega, T *x, void *stream)
{
    if (n < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_relax_jacobi_presmooth: negative size");
    if (n > INT32_MAX) return fail(CMI_ERROR_INVALID_VALUE, "cmi_relax_jacobi_presmooth: sizes exceed the int32 index type");
    if (n > 0 && (!d || !b || !x)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_relax_jacobi_presmooth: null array");
    if (n == 0) return CMI_SUCCESS;
    hipLaunchKernelGGL((jacobi_presmooth_kernel<T>), dim3(amg_blocks(n)), dim3(kAmgBlock), 0, as_stream(stream), n, d, b, omega, x);
    CMI_LAUNCH_CHECK("relax_jacobi_presmooth");
    return CMI_SUCCESS;
}

// ---- (c) tentative prolongator for one candidate vector ---------------------------------------------------------------------
// key[i] = the aggregate of row i, num_aggregates where it has none; keep[i] = 1 / 0 (keep[n] = 0); *bad = 1 on an id outside
// [-1, num_aggregates) (a plain store: every offender stores the same word)
__global__ void __launch_bounds__(kAmgBlock)
fit_keys_kernel(int64_t n, int64_t num_aggregates, const int *__restrict__ aggregates, uint32_t *__restrict__ key, int *__restrict__ keep, int *__restrict__ bad)
{
    const int64_t i = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (i > n) return;
    if (i == n) {
        keep[i] = 0;
        return;
    }
    const int a = aggregates[i];
    const bool in = a >= 0 && (int64_t)a < num_aggregates;
    if (!in && a != -1) *bad = 1;
    key[i] = in ? (uint32_t)a : (uint32_t)num_aggregates;
    keep[i] = in ? 1 : 0;
}

// ONE lane per aggregate a: its rows are the segment of the sorted keys equal to a, in ascending row order (the sort is
// stable and the rows went in ascending); the chain starts from the first square, not from +0.  No row: R[a] = 0.
template <typename T>
__global__ void __launch_bounds__(kAmgBlock)
fit_norms_kernel(int64_t n, int64_t num_aggregates, const uint32_t *__restrict__ keys, const uint32_t *__restrict__ rows, const T *__restrict__ B, T *__restrict__ R)
{
    const int64_t a = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (a >= num_aggregates) return;
    int64_t lo = 0, hi = n; // the first q with keys[q] >= a
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)keys[mid] < a) lo = mid + 1;
        else hi = mid;
    }
    T r = T(0);
    if (lo < n && (int64_t)keys[lo] == a) {
        const T b0 = B[rows[lo]];
        T s = b0 * b0;
        for (int64_t q = lo + 1; q < n && (int64_t)keys[q] == a; q++) {
            const T b = B[rows[q]];
            s = s + b * b;
        }
        r = amg_sqrt(s);
    }
    R[a] = r;
}

// one lane per row: its entry of T, if it has one
template <typename T>
__global__ void __launch_bounds__(kAmgBlock)
fit_fill_kernel(int64_t n, int64_t num_aggregates, const int *__restrict__ aggregates, const T *__restrict__ B, const T *__restrict__ R, const int *__restrict__ Tp,
                int *__restrict__ Tj, T *__restrict__ Tx, int64_t capacity)
{
    const int64_t i = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (i >= n) return;
    const int a = aggregates[i];
    if (a < 0 || (int64_t)a >= num_aggregates) return;
    const int64_t at = Tp[i];
    if (at >= capacity) return;
    Tj[at] = a;
    Tx[at] = B[i] / R[a];
}

static int amg_bits_for(int64_t count) // how many low bits hold every value in [0, count)
{
    int b = 1;
    while (b < 32 && ((int64_t)1 << b) < count) b++;
    return b;
}

template <typename T>
static int aggregates_fit(int64_t n, int64_t num_aggregates, const int *aggregates, const T *B, int *Tp, int *Tj, T *Tx, int64_t capacity, T *R, void *stream)
{
    if (n < 0 || num_aggregates < 0 || capacity < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_aggregates_fit: negative size");
    if (n > kAmgCeiling || num_aggregates > INT32_MAX - 1) return fail(CMI_ERROR_INVALID_VALUE, "cmi_aggregates_fit: sizes exceed the int32 index type");
    if (capacity < n) {
        set_error("cmi_aggregates_fit: capacity %lld is below the %lld rows", (long long)capacity, (long long)n);
        return CMI_ERROR_INVALID_VALUE;
    }
    if (!Tp || (n > 0 && (!aggregates || !B || !Tj || !Tx)) || (num_aggregates > 0 && !R)) return fail(CMI_ERROR_INVALID_VALUE, "cmi_aggregates_fit: null array");
    hipStream_t s = as_stream(stream);
    if (n == 0) {
        CMI_HIP(hipMemsetAsync(Tp, 0, sizeof(int), s));
        if (num_aggregates > 0) CMI_HIP(hipMemsetAsync(R, 0, (size_t)num_aggregates * sizeof(T), s));
        CMI_HIP(hipStreamSynchronize(s));
        return CMI_SUCCESS;
    }
    device_array<uint32_t> key_block, key_sorted_block, rows_block;
    device_array<int> keep_block;
    device_counters<int> bad; // (zeroed below, behind the other allocations)
    device_array<unsigned char> temp, scan_temp;
    size_t temp_bytes = 0;
    rocprim::counting_iterator<uint32_t> position(0);
    const unsigned end_bit = (unsigned)amg_bits_for(num_aggregates + 1);
    hipError_t e = key_block.alloc((size_t)n);
    if (e == hipSuccess) e = key_sorted_block.alloc((size_t)n);
    if (e == hipSuccess) e = rows_block.alloc((size_t)n);
    if (e == hipSuccess) e = keep_block.alloc((size_t)n + 1);
    if (e == hipSuccess) e = bad.block.alloc(1);
    uint32_t *const key = key_block.get(), *const key_sorted = key_sorted_block.get(), *const rows = rows_block.get();
    int *const keep = keep_block.get();
    // sized and allocated here, run behind the check of the ids: nothing of the caller's is touched before every block is there
    auto sort = [&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, (const uint32_t *)key, key_sorted, position, rows, (unsigned)n, 0u, end_bit, s); };
    if (e == hipSuccess) e = temp_size(sort, &temp_bytes);
    if (e == hipSuccess) e = temp.alloc(temp_bytes);
    if (e != hipSuccess) return hip_fail(e, "cmi_aggregates_fit: scratch");
    e = hipMemsetAsync(bad.dev(), 0, sizeof(int), s);
    if (e == hipSuccess) e = launch(fit_keys_kernel, amg_blocks(n + 1), kAmgBlock, 0, s, n, num_aggregates, aggregates, key, keep, bad.dev());
    if (e == hipSuccess) e = bad.fetch(s); // the flag is read once, before anything of the caller's is written
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s); // (the blocks go when this returns)
        return hip_fail(e, "cmi_aggregates_fit: checking the aggregate ids");
    }
    if (bad.host[0]) return fail(CMI_ERROR_INVALID_VALUE, "cmi_aggregates_fit: an aggregate id lies outside [-1, num_aggregates)");
    e = sort(temp.get(), temp_bytes);
    if (e == hipSuccess) e = exclusive_offsets(scan_temp, keep, Tp, n, s);
    if (e == hipSuccess && num_aggregates > 0) e = launch(fit_norms_kernel<T>, amg_blocks(num_aggregates), kAmgBlock, 0, s, n, num_aggregates, key_sorted, rows, B, R);
    if (e == hipSuccess && num_aggregates > 0) e = launch(fit_fill_kernel<T>, amg_blocks(n), kAmgBlock, 0, s, n, num_aggregates, aggregates, B, R, Tp, Tj, Tx, capacity);
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    return e == hipSuccess ? CMI_SUCCESS : hip_fail(e, "cmi_aggregates_fit");
}

// ---- (d) C = A + B, C = A - B -----------------------------------------------------------------------------------------------
// One lane per row merges the two sorted rows.  C(i,j) = the chain over A's entries at (i,j) in storage order, then B's (each
// negated first when NEGATE), started from the first of them; a result that compares equal to zero is dropped, NaN is kept.
// FILL == false: count[i] = entries of C's row i, and *unsorted = 1 when a row's offsets decrease or leave [0, entries] or its
// columns decrease or leave [0, num_cols).  FILL == true: the row is written from Cp[i] on.
template <typename T, bool FILL>
__global__ void __launch_bounds__(kAmgBlock)
elementwise_kernel(int64_t num_rows, int64_t num_cols, int64_t a_entries, const int *__restrict__ Ap, const int *__restrict__ Aj, const T *__restrict__ Ax,
                   int64_t b_entries, const int *__restrict__ Bp, const int *__restrict__ Bj, const T *__restrict__ Bx, int negate, int *__restrict__ count,
                   int *__restrict__ unsorted, const int *__restrict__ Cp, int *__restrict__ Cj, T *__restrict__ Cx, int64_t capacity)
{
    const int64_t row = (int64_t)blockIdx.x * kAmgBlock + threadIdx.x;
    if (row > num_rows) return;
    if (row == num_rows) {
        if (!FILL) {
            count[row] = 0;
            if (Ap[row] != (int)a_entries || Bp[row] != (int)b_entries || Ap[0] != 0 || Bp[0] != 0) *unsorted = 1;
        }
        return;
    }
    const int a0 = Ap[row], a1 = Ap[row + 1], b0 = Bp[row], b1 = Bp[row + 1];
    int ia = amg_clamp(a0, a_entries), ea = amg_clamp(a1, a_entries), ib = amg_clamp(b0, b_entries), eb = amg_clamp(b1, b_entries);
    if (ea < ia) ea = ia;
    if (eb < ib) eb = ib;
    bool ok = a0 == ia && a1 == ea && b0 == ib && b1 == eb;
    int64_t at = FILL ? (int64_t)Cp[row] : 0;
    int n = 0;
    int prev = -1;
    while (ia < ea || ib < eb) {
        const int ca = ia < ea ? Aj[ia] : INT32_MAX, cb = ib < eb ? Bj[ib] : INT32_MAX;
        const int c = ca < cb ? ca : cb;
        if (c < prev || c < 0 || (int64_t)c >= num_cols) ok = false;
        prev = c;
        T s = T(0);
        bool first = true;
        while (ia < ea && Aj[ia] == c) {
            const T v = Ax[ia++];
            s = first ? v : s + v;
            first = false;
        }
        while (ib < eb && Bj[ib] == c) {
            T v = Bx[ib++];
            if (negate) v = -v;
            s = first ? v : s + v;
            first = false;
        }
        if (!(s == T(0))) {
            if (FILL && at + n < capacity) {
                Cj[at + n] = c;
                Cx[at + n] = s;
            }
            n++;
        }
    }
    if (!FILL) {
        count[row] = n;
        if (!ok) *unsorted = 1;
    }
}

template <typename T>
static int csr_elementwise(int64_t num_rows, int64_t num_cols, int64_t a_entries, const int *Ap, const int *Aj, const T *Ax, int64_t b_entries, const int *Bp,
                           const int *Bj, const T *Bx, int op, int *Cp, int *Cj, T *Cx, int64_t capacity, int *sorted_host, void *stream)
{
    if (num_rows < 0 || num_cols < 0 || a_entries < 0 || b_entries < 0 || capacity < 0) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_elementwise: negative size");
    if (num_rows > INT32_MAX - 1 || num_cols > INT32_MAX - 1 || a_entries > kAmgCeiling || b_entries > kAmgCeiling || a_entries + b_entries > kAmgCeiling)
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_elementwise: sizes exceed the int32 index type");
    if (op != 0 && op != 1) return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_elementwise: op is 0 (add) or 1 (subtract)");
    if (capacity < a_entries + b_entries) {
        set_error("cmi_csr_elementwise: capacity %lld is below the %lld entries of A plus B", (long long)capacity, (long long)(a_entries + b_entries));
        return CMI_ERROR_INVALID_VALUE;
    }
    if (!sorted_host || !Cp || !Ap || !Bp || (a_entries > 0 && (!Aj || !Ax)) || (b_entries > 0 && (!Bj || !Bx)) || (a_entries + b_entries > 0 && (!Cj || !Cx)))
        return fail(CMI_ERROR_INVALID_VALUE, "cmi_csr_elementwise: null array");
    *sorted_host = 0;
    hipStream_t s = as_stream(stream);
    device_array<int> count_block;
    device_counters<int> unsorted;
    device_array<unsigned char> scan_temp;
    hipError_t e = count_block.alloc((size_t)num_rows + 1);
    if (e == hipSuccess) e = unsorted.block.alloc(1);
    if (e != hipSuccess) return hip_fail(e, "cmi_csr_elementwise: scratch");
    int *const count = count_block.get();
    e = hipMemsetAsync(unsorted.dev(), 0, sizeof(int), s);
    if (e == hipSuccess)
        e = launch(elementwise_kernel<T, false>, amg_blocks(num_rows + 1), kAmgBlock, 0, s, num_rows, num_cols, a_entries, Ap, Aj, Ax, b_entries, Bp, Bj, Bx, op, count,
                   unsorted.dev(), nullptr, nullptr, nullptr, capacity);
    if (e == hipSuccess) e = unsorted.fetch(s); // the flag is read once, before anything of the caller's is written
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(s); // (the blocks go when this returns)
        return hip_fail(e, "cmi_csr_elementwise: counting");
    }
    if (unsorted.host[0]) return CMI_SUCCESS; // *sorted_host == 0: the caller sorts, or takes its host path
    e = exclusive_offsets(scan_temp, count, Cp, num_rows, s);
    if (e == hipSuccess && num_rows > 0)
        e = launch(elementwise_kernel<T, true>, amg_blocks(num_rows), kAmgBlock, 0, s, num_rows, num_cols, a_entries, Ap, Aj, Ax, b_entries, Bp, Bj, Bx, op, nullptr,
                   nullptr, Cp, Cj, Cx, capacity);
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return hip_fail(e, "cmi_csr_elementwise");
    *sorted_host = 1;
    return CMI_SUCCESS;
}

} // namespace cmi

CMI_API int cmi_csr_strength_symmetric_f64(int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *Ap, const int32_t *Aj, const double *Ax,
                                           double theta, int32_t *Sp, int32_t *Sj, double *Sx, int64_t capacity, void *stream)
{ return cmi::strength_symmetric<double>(num_rows, num_cols, num_entries, Ap, Aj, Ax, theta, Sp, Sj, Sx, capacity, stream); }
CMI_API int cmi_csr_strength_symmetric_f32(int64_t num_rows, int64_t num_cols, int64_t num_entries, const int32_t *Ap, const int32_t *Aj, const float *Ax,
                                           double theta, int32_t *Sp, int32_t *Sj, float *Sx, int64_t capacity, void *stream)
{ return cmi::strength_symmetric<float>(num_rows, num_cols, num_entries, Ap, Aj, Ax, theta, Sp, Sj, Sx, capacity, stream); }

CMI_API int cmi_csr_scale_rows_f64(int64_t num_rows, int64_t num_entries, const int32_t *Ap, const double *Ax, const double *d, double lambda, double *out,
                                   void *stream)
{ return cmi::scale_rows<double>(num_rows, num_entries, Ap, Ax, d, lambda, out, stream); }
CMI_API int cmi_csr_scale_rows_f32(int64_t num_rows, int64_t num_entries, const int32_t *Ap, const float *Ax, const float *d, float lambda, float *out, void *stream)
{ return cmi::scale_rows<float>(num_rows, num_entries, Ap, Ax, d, lambda, out, stream); }

CMI_API int cmi_aggregates_fit_f64(int64_t n, int64_t num_aggregates, const int32_t *aggregates, const double *B, int32_t *Tp, int32_t *Tj, double *Tx,
                                   int64_t capacity, double *R, void *stream)
{ return cmi::aggregates_fit<double>(n, num_aggregates, aggregates, B, Tp, Tj, Tx, capacity, R, stream); }
CMI_API int cmi_aggregates_fit_f32(int64_t n, int64_t num_aggregates, const int32_t *aggregates, const float *B, int32_t *Tp, int32_t *Tj, float *Tx,
                                   int64_t capacity, float *R, void *stream)
{ return cmi::aggregates_fit<float>(n, num_aggregates, aggregates, B, Tp, Tj, Tx, capacity, R, stream); }

CMI_API int cmi_csr_elementwise_f64(int64_t num_rows, int64_t num_cols, int64_t a_entries, const int32_t *Ap, const int32_t *Aj, const double *Ax,
                                    int64_t b_entries, const int32_t *Bp, const int32_t *Bj, const double *Bx, int op, int32_t *Cp, int32_t *Cj, double *Cx,
                                    int64_t capacity, int *sorted_host, void *stream)
{ return cmi::csr_elementwise<double>(num_rows, num_cols, a_entries, Ap, Aj, Ax, b_entries, Bp, Bj, Bx, op, Cp, Cj, Cx, capacity, sorted_host, stream); }
CMI_API int cmi_csr_elementwise_f32(int64_t num_rows, int64_t num_cols, int64_t a_entries, const int32_t *Ap, const int32_t *Aj, const float *Ax,
                                    int64_t b_entries, const int32_t *Bp, const int32_t *Bj, const float *Bx, int op, int32_t *Cp, int32_t *Cj, float *Cx,
                                    int64_t capacity, int *sorted_host, void *stream)
{ return cmi::csr_elementwise<float>(num_rows, num_cols, a_entries, Ap, Aj, Ax, b_entries, Bp, Bj, Bx, op, Cp, Cj, Cx, capacity, sorted_host, stream); }

CMI_API int cmi_relax_jacobi_presmooth_f64(int64_t n, const double *d, const double *b, double omega, double *x, void *stream)
{ return cmi::jacobi_presmooth<double>(n, d, b, omega, x, stream); }
CMI_API int cmi_relax_jacobi_presmooth_f32(int64_t n, const float *d, const float *b, float omega, float *x, void *stream)
{ return cmi::jacobi_presmooth<float>(n, d, b, omega, x, stream); }
